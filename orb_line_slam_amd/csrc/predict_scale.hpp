// predict_scale.hpp -- MapPoint::PredictScale (src/MapPoint.cc:414-429) as the host searches evaluate it, in one place: search_host.cpp predicts with it,
// and olf_predict_scale_thresholds turns this very function into the table of ratios at which its result steps, which is what the device compares against
// (csrc/local_batch.hip) -- no logarithm runs there.
#pragma once
#include <cmath>

namespace olf {

inline int predict_scale(float maxd, float dist, float logScaleFactor, int nLevels)       // MapPoint::PredictScale, src/MapPoint.cc:414-429
{
    const float ratio = maxd / dist;
    int n = (int)std::ceil(std::log(ratio) / logScaleFactor);
    if (n < 0) n = 0; else if (n >= nLevels) n = nLevels - 1;
    return n;
}

inline float log_scale_factor(const float* scale_factors, int n_levels) { return n_levels > 1 ? std::log(scale_factors[1]) : 1.0f; }    // mfLogScaleFactor

}  // namespace olf
