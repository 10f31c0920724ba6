// dense_math.hpp -- the small dense arithmetic the three optimisers' terms headers (pose_terms.hpp, posepoints_terms.hpp, optsim3_terms.hpp) share: 4 x 4
// and 3 x 3 products, se(3)'s inverse, Eigen's quaternion of a rotation and back, the quaternion product and rotation.  Plain C++ over doubles, no Eigen,
// no HIP header: the host forms are built with g++ alone.  Built with -ffp-contract=off on both sides, so the same operands give the same bits on the host
// and on the device.  An Eigen product sums over k in ascending order; a quaternion is x, y, z, w and its norm is summed in that order.
#pragma once
#include <math.h>
#include <stdint.h>

// Not OLF_HD (device_math.hpp), which forces inlining and made k_pose_frames longer and slower ("What the map-side kernels share").
#if defined(__HIPCC__)
#define PT_HD __host__ __device__ inline
#else
#define PT_HD inline
#endif

namespace olf {
namespace dense {

PT_HD bool finite_d(double x) { return x - x == 0.0; }
PT_HD double max_d(double a, double b) { return a < b ? b : a; }      // std::max(a, b)
PT_HD double min_d(double a, double b) { return b < a ? b : a; }      // std::min(a, b)

// ---- 4 x 4 and se(3), row-major ------------------------------------------------------------------------------------------------------------------------
PT_HD void mat4_identity(double* T) { for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0; }
PT_HD void mat4_mul(const double* A, const double* B, double* C)
{
    double t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = A[i * 4] * B[j];
            for (int k = 1; k < 4; ++k) s = s + A[i * 4 + k] * B[k * 4 + j];
            t[i * 4 + j] = s;
        }
    for (int i = 0; i < 16; ++i) C[i] = t[i];
}
PT_HD bool mat4_finite(const double* T) { bool ok = true; for (int i = 0; i < 16; ++i) ok = ok && finite_d(T[i]); return ok; }
// inverse_se3 (src/Auxiliar.cc:113-122) and Converter::toInvMatrix4d: R^T | -R^T t
PT_HD void inverse_se3(const double* T, double* Ti)
{
    double o[16];
    mat4_identity(o);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = T[j * 4 + i];
        o[i * 4 + 3] = ((-T[0 * 4 + i]) * T[3] + (-T[1 * 4 + i]) * T[7]) + (-T[2 * 4 + i]) * T[11];
    }
    for (int i = 0; i < 16; ++i) Ti[i] = o[i];
}
PT_HD void skew3(const double* w, double* S)
{
    S[0] = 0.0; S[1] = -w[2]; S[2] = w[1];
    S[3] = w[2]; S[4] = 0.0; S[5] = -w[0];
    S[6] = -w[1]; S[7] = w[0]; S[8] = 0.0;
}
PT_HD void mat3_mul(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}
PT_HD void mat3_vec(const double* A, const double* v, double* o)
{
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = (A[i * 3] * v[0] + A[i * 3 + 1] * v[1]) + A[i * 3 + 2] * v[2];
    o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
}

// ---- quaternions, x, y, z, w ---------------------------------------------------------------------------------------------------------------------------
// g2o::SE3Quat(R, t)'s rotation (se3quat.h:58-60, :280-285): Eigen's Quaterniond(R) of the rotation block of the row-major 4 x 4 T, then
// normalizeRotation(), i.e. w >= 0 and unit norm.
PT_HD void quat_normalize_positive(double* q)
{
    if (q[3] < 0.0) for (int i = 0; i < 4; ++i) q[i] = q[i] * -1.0;
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
}
// Eigen's Quaterniond(Matrix3d) of the 3 x 3 block at M (row-major, rows ld apart), NOT normalised (what g2o::Sim3 keeps; optsim3_terms.hpp)
PT_HD void quat_of_rotation(const double* M, int ld, double* q)
{
    const int dg = ld + 1;
    const double m00 = M[0], m11 = M[dg], m22 = M[2 * dg];
    double t = (m00 + m11) + m22;
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (M[2 * ld + 1] - M[ld + 2]) * t; q[1] = (M[2] - M[2 * ld]) * t; q[2] = (M[ld] - M[1]) * t;
    } else {
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > M[i * dg]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(((M[i * dg] - M[j * dg]) - M[k * dg]) + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (M[k * ld + j] - M[j * ld + k]) * t;
        q[j] = (M[j * ld + i] + M[i * ld + j]) * t;
        q[k] = (M[k * ld + i] + M[i * ld + k]) * t;
    }
}
PT_HD void quat_from_mat4(const double* T, double* q)
{
    quat_of_rotation(T, 4, q);
    quat_normalize_positive(q);
}
// Quaterniond::toRotationMatrix(), row-major 3 x 3
PT_HD void quat_to_mat3(const double* q, double* R)
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1],
                 tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
PT_HD void cross3(const double* a, const double* b, double* o)
{
    const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    o[0] = x; o[1] = y; o[2] = z;
}
// Quaterniond * Vector3d (Eigen's _transformVector): v + w * uv + vec x uv with uv = 2 (vec x v)
PT_HD void quat_rotate(const double* q, const double* v, double* o)
{
    double uv[3], c[3];
    cross3(q, v, uv);
    for (int i = 0; i < 3; ++i) uv[i] = uv[i] + uv[i];
    cross3(q, uv, c);
    for (int i = 0; i < 3; ++i) o[i] = (v[i] + q[3] * uv[i]) + c[i];
}
// Quaterniond * Quaterniond, the generic (not the SSE) product; o may not alias a or b
PT_HD void quat_mul(const double* a, const double* b, double* o)
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    o[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    o[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    o[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
    o[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
}

}  // namespace dense
}  // namespace olf
