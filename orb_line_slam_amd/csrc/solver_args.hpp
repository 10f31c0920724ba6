// solver_args.hpp -- what every form of the RANSAC solvers (the _dev entries of sim3solver_batch.hip / pnpsolver_batch.hip / initializer_batch.hip, the host
// forms *_host.cpp and the staged forms *_api.cpp) checks of its caller's parameter block and of its io block, declared once; each is defined once, in its solver's host form.
// Plain C++: the host forms are also built without the library.
#pragma once
#include "../../include/orbline.h"

namespace olf {

bool sim3_ransac_ok(const olf_sim3_ransac* R);      // sim3solver_host.cpp: not NULL, min_inliers >= 3, max_iterations >= 1, n_iterations >= 0, 0 < probability < 1
bool sim3_io_ok(const olf_sim3_solver_io* io);      // not NULL, and every array but `counts`
bool pnp_ransac_ok(const olf_pnp_ransac* R);        // pnpsolver_host.cpp: as above with min_inliers >= 1, and min_set == 4, 0 < epsilon <= 1, th2 > 0
bool pnp_io_ok(const olf_pnp_solver_io* io);
// the initialiser's (initializer_host.cpp): sigma > 0 and finite, max_iterations >= 1, min_triangulated >= 0, min_parallax finite; every array of io.
// ini_cos_threshold is C.34's: the largest float cosine whose parallax in degrees is > (strict) or >= min_parallax under this machine's acosf (NaN: none);
// false: the comparison is not monotone around it
bool ini_params_ok(const olf_initializer_params* P);
bool ini_io_ok(const olf_initializer_io* io);
bool ini_cos_threshold(float min_parallax, bool strict, float* out);

inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace olf
