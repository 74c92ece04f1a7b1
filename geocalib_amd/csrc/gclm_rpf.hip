// gclm_rpf.hip -- gclm_rpf_hypotheses: the three-pixel minimal solver of the reference's RANSAC baseline
// (siclib/models/optimization/ransac.py: MinimalSolver, RPFSolver.solve_rpf), one lane per sample.  What it produces are
// the rows gclm_hypothesis_scores ranks: cameras (B, N Rn, 8) and gravities (B, N Rn, 3), invalid rows all NaN.
//
// The definition (include/gclm.h states it in full; DESIGN.md 3.11 says where and why it leaves the reference):
//   pixels 0, 1: the lines through (x_k, y_k) along the up vector d_k meet in the vertical vanishing point V = l_0 x l_1,
//                kept homogeneous; v = (V_x - c_x V_z, V_y - c_y V_z, V_z) / |.| is (f g_x, f g_y, g_z) up to scale
//   pixel 2:     L = sin(latitude) gives a0 F^2 + a1 F + a2 = 0 in F = f^2, solved with q = -(a1 + sgn(a1) sqrt(disc)) / 2,
//                roots a2 / q and q / a0; with a prior focal length F = prior^2 and the latitude is not read
//   per root:    f = sqrt(F), g = normalize(v_x / f, v_y / f, v_z), its sign from the up DIRECTION at pixel 0; valid iff f
//                and g are finite, f lies in the LM's focal clamp and (without a prior) the unsquared latitude equation holds
//                in sign.
// Floating-point contraction is OFF for the solver: a2 = L^2 R S - D^2 and the discriminant cancel, and the torch
// composition of geocalib_amd/ransac.py, which states the same operations one by one, is the yardstick of the measurement.
//
// Layout: grid = (ceil(N / 256), B), one lane per sample, five gathered loads per lane (two up vectors, one latitude; the
// six sample coordinates are read from d_samples or drawn in the lane), 11 Rn stores; no LDS, no atomics, no scratch; one
// row index per lane, 64-bit offsets.  A sample whose coordinates lie outside the image reads nothing and leaves invalid rows.
#include "gclm_internal.h"

namespace gclm {
namespace {

constexpr int kRpfBlock = 256;

// the splitmix64 finaliser (as gclm_synth.hip has it: restated, the synthetic generator's bits are its own)
__device__ __forceinline__ uint64_t rpf_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct RpfArgs {
    const float *up, *lat, *prior;
    const int32_t* samples;
    uint64_t seed;
    int64_t first;
    int N, H, W;
    float *cam, *grav;
    int32_t* samples_out;
};

struct RpfRow { float f, gx, gy, gz; };

#pragma clang fp contract(off)
// One root: F = f^2 -> the row, NaN where it is invalid.  (U, Vp), L: pixel 2; (U0, V0), (d0x, d0y): pixel 0.
template <bool PRIOR>
__device__ __forceinline__ RpfRow rpf_root(float F, float vx, float vy, float vz, float U, float Vp, float L, float U0, float V0,
                                           float d0x, float d0y, float fmin, float fmax) {
    const float f = sqrtf(F);
    float gx = vx / f, gy = vy / f, gz = vz;
    const float n = sqrtf(gx * gx + gy * gy + gz * gz);
    gx /= n, gy /= n, gz /= n;
    const float dot = (gx - gz * (U0 / f)) * d0x + (gy - gz * (V0 / f)) * d0y;
    if (dot < 0.f) gx = -gx, gy = -gy, gz = -gz;
    // (every comparison is false for a NaN: a NaN anywhere leaves the row invalid)
    bool valid = f >= fmin && f <= fmax && fabsf(gx) + fabsf(gy) + fabsf(gz) <= 2.f;         // (|g|_1 <= sqrt 3 for a unit g)
    if (!PRIOR) valid = valid && L * (gx * (U / f) + gy * (Vp / f) + gz) >= 0.f;
    const float nan = __builtin_nanf("");
    return valid ? RpfRow{f, gx, gy, gz} : RpfRow{nan, nan, nan, nan};
}

template <bool PRIOR>
__global__ __launch_bounds__(kRpfBlock) void rpf_kernel(const RpfArgs a) {
    constexpr int Rn = PRIOR ? 1 : 2;
    const int n = blockIdx.x * kRpfBlock + threadIdx.x, b = blockIdx.y;
    if (n >= a.N) return;
    const size_t row = (size_t)b * a.N + n;       // the one row index of the lane
    int x[3], y[3];
    if (a.samples) {
        const int32_t* s = a.samples + row * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = s[2 * k], y[k] = s[2 * k + 1];
    } else {
        // pixel k of sample n of image i = first_index + b: one 64-bit hash, x from its high and y from its low 32 bits
        const uint64_t i = (uint64_t)a.first + (uint64_t)b;
        const uint64_t base = rpf_mix64((a.seed ^ GCLM_RPF_DRAW_SALT) ^ rpf_mix64(i * 0xD1342543DE82EF95ull + 1));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint64_t h = rpf_mix64(base + (uint64_t)n * 4 + k);
            x[k] = (int)(((h >> 32) * (uint64_t)a.W) >> 32);
            y[k] = (int)(((h & 0xFFFFFFFFull) * (uint64_t)a.H) >> 32);
        }
    }
    if (a.samples_out) {
        int32_t* s = a.samples_out + row * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[2 * k] = x[k], s[2 * k + 1] = y[k];
    }
    const float nan = __builtin_nanf("");
    RpfRow r[Rn];
#pragma unroll
    for (int j = 0; j < Rn; ++j) r[j] = RpfRow{nan, nan, nan, nan};
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) inside = inside && x[k] >= 0 && x[k] < a.W && y[k] >= 0 && y[k] < a.H;
    if (inside) {
        const size_t hw = (size_t)a.H * a.W;
        const float* up = a.up + (size_t)b * 2 * hw;
        const size_t o0 = (size_t)y[0] * a.W + x[0], o1 = (size_t)y[1] * a.W + x[1];
        const float d0x = up[o0], d0y = up[hw + o0], d1x = up[o1], d1y = up[hw + o1];
        const float cx = 0.5f * (float)a.W, cy = 0.5f * (float)a.H;
        const float x0 = (float)x[0], y0 = (float)y[0], x1 = (float)x[1], y1 = (float)y[1];
        // l_k = (-d_ky, d_kx, x_k d_ky - y_k d_kx),  V = l_0 x l_1
        const float l0x = -d0y, l0y = d0x, l0z = x0 * d0y - y0 * d0x;
        const float l1x = -d1y, l1y = d1x, l1z = x1 * d1y - y1 * d1x;
        const float Vx = l0y * l1z - l0z * l1y, Vy = l0z * l1x - l0x * l1z, Vz = l0x * l1y - l0y * l1x;
        float vx = Vx - cx * Vz, vy = Vy - cy * Vz, vz = Vz;
        const float vn = sqrtf(vx * vx + vy * vy + vz * vz);
        vx /= vn, vy /= vn, vz /= vn;
        const float U = (float)x[2] - cx, Vp = (float)y[2] - cy, U0 = x0 - cx, V0 = y0 - cy;
        const float fmin = (float)a.H * 0.5f / 3.7320504f, fmax = (float)a.H * 0.5f / 0.043660942f;     // the LM's clamp (gclm_device.h)
        if constexpr (PRIOR) {
            const float p = a.prior[b];
            r[0] = rpf_root<true>(p * p, vx, vy, vz, U, Vp, 0.f, U0, V0, d0x, d0y, fmin, fmax);
        } else {
            const float L = sinf(a.lat[(size_t)b * hw + (size_t)y[2] * a.W + x[2]]);
            const float L2 = L * L, R = U * U + Vp * Vp, S = vx * vx + vy * vy, D = vx * U + vy * Vp, vz2 = vz * vz;
            const float a0 = (L2 - 1.f) * vz2;
            const float a1 = L2 * (R * vz2 + S) - 2.f * D * vz;
            const float a2 = L2 * R * S - D * D;
            const float root = sqrtf(a1 * a1 - 4.f * a0 * a2);
            const float q = -(a1 + (a1 >= 0.f ? root : -root)) / 2.f;
            r[0] = rpf_root<false>(a2 / q, vx, vy, vz, U, Vp, L, U0, V0, d0x, d0y, fmin, fmax);
            r[1] = rpf_root<false>(q / a0, vx, vy, vz, U, Vp, L, U0, V0, d0x, d0y, fmin, fmax);
        }
    }
    const float w = (float)a.W, h = (float)a.H;
#pragma unroll
    for (int j = 0; j < Rn; ++j) {
        const bool ok = r[j].f == r[j].f;
        float* c = a.cam + (row * Rn + j) * 8;
        float* g = a.grav + (row * Rn + j) * 3;
        c[0] = ok ? w : nan, c[1] = ok ? h : nan, c[2] = r[j].f, c[3] = r[j].f;
        c[4] = ok ? 0.5f * w : nan, c[5] = ok ? 0.5f * h : nan, c[6] = ok ? 0.f : nan, c[7] = ok ? 0.f : nan;
        g[0] = r[j].gx, g[1] = r[j].gy, g[2] = r[j].gz;
    }
}

}  // namespace

hipError_t launch_rpf_hypotheses(const float* up, const float* lat, const float* prior_focal, const int32_t* samples, uint64_t seed,
                                 int64_t first_index, int B, int N, int H, int W, float* cam, float* grav, int32_t* samples_out,
                                 hipStream_t st) {
    const RpfArgs a{up, lat, prior_focal, samples, seed, first_index, N, H, W, cam, grav, samples_out};
    const dim3 grid((N + kRpfBlock - 1) / kRpfBlock, B);
    if (prior_focal)
        hipLaunchKernelGGL(rpf_kernel<true>, grid, dim3(kRpfBlock), 0, st, a);
    else
        hipLaunchKernelGGL(rpf_kernel<false>, grid, dim3(kRpfBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace gclm
