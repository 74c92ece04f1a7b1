// gclm_param_opt.hip -- gclm_param_opt, gclm_param_opt_cost, gclm_param_opt_step: Adam on (roll, pitch, vfov) of a pinhole
// camera against predicted perspective fields, per image (the reference's PerspectiveParamOpt,
// siclib/models/optimization/perspective_opt.py, which takes one image per call, renders both fields and differentiates them
// with autograd every step).  Here a step is one streaming pass over the three planes and one small launch per batch.
//
// Per image the state is (r, p, v) = (roll, pitch, vfov), from which g = (a, b, c) = (-sin r cos p, -cos r cos p, sin p),
// f = (H / 2) / tan(v / 2), the principal point (W / 2, H / 2) and integer pixel centres: u = (x - W / 2) / f, w = (y - H / 2) / f.
//
// The pass (param_opt_pass_kernel), per pixel with the targets t (up) and l (latitude):
//   up:   q = (a - c u, b - c w), U = q / |q|, T = t / max(|t|, 1e-8) (torch's cosine_similarity);
//         theta = atan2(|U x T|, U . T) -- gclm_render.h's form of acos(U . T), which resolves small angles in float32 -- held to
//         [theta_clip, pi - theta_clip], theta_clip = acos(1 - 1e-7): the reference's clip of the cosine.  Inside the clip the
//         cost is the constant and the gradient 0; elsewhere, for a parameter s,
//         d theta / ds = -sign(U x T) (n . dq/ds) / |q|,  n = (-U_y, U_x):  for unit vectors the angle changes at exactly the
//         angular rate of U -- no 1 / sqrt(1 - cos^2), hence no division by a rounded cosine next to 1.
//   lat:  s = (a u + b w + c) / sqrt(u^2 + w^2 + 1), clamped as persp_lat clamps it; e = |asin(s) - l|;
//         de/ds' = sign(asin(s) - l) ds/ds' / sqrt(1 - s^2), 0 where the clamp is active.
//   dg/dr = (-cos r cos p, sin r cos p, 0), dg/dp = (sin r sin p, cos r sin p, cos p) (Gravity.J_rp's tangent columns),
//   dq/df = c (u, w) / f,  ds/df = -((a u + b w) - s (u^2 + w^2) / n) / (f n),  df/dv = -(H / 4) / sin^2(v / 2).
// The per-image terms (g, its two tangent columns, 1 / f, the principal point) are formed ONCE per image in float64, by the lane
// that moved the state, and left as a 16-float pose record the pass reads with uniform loads; the factors of the focal
// derivative that do not depend on the pixel (c / f, -1 / f, df/dv) are applied after the sum, in float64.
//
// Reduction: the tile walk of gclm_render.h ("The tile walk"), with one record of eight floats per workgroup in the caller's
// workspace [sum theta, sum e, three sums of d theta, three of d e]; param_opt_finish_kernel (one block per image) sums an
// image's records in 32 chains.  No atomics on floats: an image's bits depend on its pixels, H, W and the pixels per lane
// alone -- not on B, not on the other images.
//
// The update (param_opt_update, one lane per image) is the reference's step in its order: Adam (torch's defaults, bias
// corrections; parameters and moments float32, the arithmetic of one step in float64 and rounded once), then
// ReduceLROnPlateau.step(loss), then check_convergence(loss); include/gclm.h has the state record and every branch.
// Every deciding comparison is made in float64 on the float32 loss, as Python does with .item().  A converged image's
// record freezes; its workgroups return after one uniform load.
#include "gclm_render.h"

namespace gclm {
namespace {

constexpr int kRecWords = 8;                  // floats per workgroup record
constexpr int kChains = 32;                   // summation chains per image of the finish
constexpr int kPoseWords = 16;                // floats per pose record: a b c 1/f | dg/dr (x, y) | dg/dp (x, y, z) | cx cy | pad
constexpr int kStateWords = GCLM_PARAM_OPT_STATE_WORDS;
constexpr int kInfoWords = GCLM_PARAM_OPT_INFO_WORDS;
constexpr float kThetaClip = 4.4721359922676e-4f;          // acos(1 - 1e-7)
constexpr float kPiF = 3.14159265358979323846f;

// words of the state record (include/gclm.h: gclm_param_opt_step)
enum { S_RPV = 0, S_M = 3, S_V = 6, S_STEPS = 9, S_DONE = 10, S_BAD = 11, S_COOL = 12, S_WLEN = 13, S_LR = 14, S_BEST = 16,
       S_TOTAL = 17, S_UP = 18, S_LAT = 19, S_WINDOW = 20, S_INIT = 28 };

struct ParamOptCfg {                          // gclm_param_opt_config without its stamp
    int patience, use_sched, sched_patience, sched_cooldown;
    double lr, abs_tol, rel_tol, lamb, factor, threshold, min_lr, eps;
};

struct PassArgs {
    const float *up, *lat, *pose;
    const int32_t* done;                      // word S_DONE of image 0's state record, or NULL: every image is live
    float* rec;
    int H, W, tiles_x;
};

// 1 / sqrt(x) as one instruction (v_rsq_f32, 1 ulp): the pass is bound by arithmetic, and the IEEE square root and division it
// stands for cost some twenty instructions.  Its rounding is per pixel and averages out in the sums (tests/test_param_opt.py).
__device__ __forceinline__ float rsq(float x) { return __frsqrt_rn(x); }

template <int PX>
__global__ __launch_bounds__(kBlock) void param_opt_pass_kernel(const PassArgs a) {
    __shared__ float s_sum[kTileRows][kRecWords];
    const int b = blockIdx.y, wave = threadIdx.x >> 6;
    if (a.done && a.done[(size_t)b * kStateWords]) return;        // (uniform: the whole block leaves)
    int x, y;
    const bool in = tile_pixel<PX>(a.tiles_x, a.H, a.W, x, y);
    float sum[kRecWords] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) {
        const float* P = a.pose + (size_t)b * kPoseWords;
        const float ga = P[0], gb = P[1], gc = P[2], ifx = P[3], dar = P[4], dbr = P[5], dap = P[6], dbp = P[7], dcp = P[8];
        const float w = ((float)y - P[10]) * ifx, w2 = w * w, qy = gb - gc * w;
        const size_t hw = (size_t)a.H * a.W, o = (size_t)b * hw + (size_t)y * a.W + x;
        float tx[PX], ty[PX], tl[PX];
        load_px<PX>(a.up + o + (size_t)b * hw, tx);              // (B, 2, H, W): image b starts at 2 b H W
        load_px<PX>(a.up + o + (size_t)b * hw + hw, ty);
        load_px<PX>(a.lat + o, tl);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float u = ((float)(x + j) - P[9]) * ifx;
            {   // up
                const float qx = ga - gc * u, n2 = qx * qx + qy * qy;
                const float iq = n2 < 1e-24f ? 1e12f : rsq(n2);   // 1 / max(|q|, 1e-12), F.normalize's clamp_min; a NaN stays NaN
                const float ux = qx * iq, uy = qy * iq;
                const float tn2 = tx[j] * tx[j] + ty[j] * ty[j];
                float dot = ux * tx[j] + uy * ty[j], crs = ux * ty[j] - uy * tx[j], sn, wgt;
                if (tn2 >= kCosEps * kCosEps) {
                    const float it = rsq(tn2);
                    dot *= it, crs *= it;
                    sn = fabsf(crs);
                    wgt = crs > 0.f ? -1.f : (crs < 0.f ? 1.f : crs * 0.f);     // -sign(U x T); NaN stays NaN
                } else {                      // a target shorter than eps (or NaN): the cosine of a vector shorter than 1
                    float tn = sqrtf(tn2);
                    tn = tn < kCosEps ? kCosEps : tn;
                    const float it = 1.f / tn, gap = 1.f - tn2 * it * it;
                    dot *= it, crs *= it;
                    sn = sqrtf((gap > 0.f ? gap : 0.f) + crs * crs);
                    wgt = -crs / sn;
                }
                float th = atan2f(sn, dot);
                const bool lo = th < kThetaClip, hi = th > kPiF - kThetaClip;
                const float m = (lo || hi) ? 0.f : wgt * iq;                    // NaN: no clip, the gradient is NaN
                th = lo ? kThetaClip : (hi ? kPiF - kThetaClip : th);
                sum[0] += th;
                sum[2] += m * (ux * dbr - uy * dar);                            // n . dq/dr, n = (-uy, ux)
                sum[3] += m * (ux * (dbp - dcp * w) - uy * (dap - dcp * u));
                sum[4] += m * (ux * w - uy * u);                                // times c / f, after the sum
            }
            {   // latitude
                const float r2 = u * u + w2, inn = rsq(r2 + 1.f), lin = ga * u + gb * w;
                const float s = (lin + gc) * inn;
                const bool clamped = s < -kLatHi || s > kLatHi;
                const float sc = s < -kLatHi ? -kLatHi : (s > kLatHi ? kLatHi : s);     // a NaN stays NaN
                const float d = asinf(sc) - tl[j];
                const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : d * 0.f);            // sign(0) = 0, NaN stays NaN
                const float k = clamped ? 0.f : sg * inn * rsq((1.f - s) * (1.f + s));
                sum[1] += fabsf(d);
                sum[5] += k * (dar * u + dbr * w);
                sum[6] += k * (dap * u + dbp * w + dcp);
                sum[7] += k * (lin - s * r2 * inn);                             // times -1 / f, after the sum
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kRecWords; ++k) sum[k] = wave_sum(sum[k]);
    tile_record(s_sum, wave, sum, [&](int k, float s) { a.rec[((size_t)b * gridDim.x + blockIdx.x) * kRecWords + k] = s; });
}

// The pose record of a state, formed in float64 and rounded once.
__device__ void write_pose(const float* rpv, int H, int W, float* pose) {
    const double r = rpv[0], p = rpv[1], v = rpv[2];
    const double sr = sin(r), cr = cos(r), sp = sin(p), cp = cos(p), f = 0.5 * H / tan(0.5 * v);
    const float out[kPoseWords] = {(float)(-sr * cp), (float)(-cr * cp), (float)sp, (float)(1.0 / f), (float)(-cr * cp), (float)(sr * cp),
                                   (float)(sr * sp), (float)(cr * sp), (float)cp, 0.5f * W, 0.5f * H, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < kPoseWords; ++k) pose[k] = out[k];
}

// One update of one image's state record from the eight numbers of the pass (file header; include/gclm.h).
__device__ void param_opt_update(uint32_t* s, const float* cost, const ParamOptCfg& c) {
    float* f = reinterpret_cast<float*>(s);
    int32_t* n = reinterpret_cast<int32_t*>(s);
    double& lr = *reinterpret_cast<double*>(s + S_LR);
    const float total = (float)(c.lamb * (double)cost[1] + (1.0 - c.lamb) * (double)cost[0]);
    const double cur = total;
    // Adam
    const int t = ++n[S_STEPS];
    const double b1 = 0.9, b2 = 0.999, bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    const double step_size = lr / bc1, bc2_sqrt = sqrt(bc2);
    for (int j = 0; j < 3; ++j) {
        const float g = (float)(c.lamb * (double)cost[5 + j] + (1.0 - c.lamb) * (double)cost[2 + j]);
        const float m = (float)((double)f[S_M + j] + ((double)g - (double)f[S_M + j]) * (1.0 - b1));
        const float v = (float)((double)f[S_V + j] * b2 + (1.0 - b2) * (double)g * (double)g);
        f[S_M + j] = m, f[S_V + j] = v;
        f[S_RPV + j] = (float)((double)f[S_RPV + j] - step_size * ((double)m / (sqrt((double)v) / bc2_sqrt + 1e-8)));
    }
    // ReduceLROnPlateau.step(loss), mode "min", threshold_mode "rel"
    if (c.use_sched) {
        if (cur < (double)f[S_BEST] * (1.0 - c.threshold)) f[S_BEST] = total, n[S_BAD] = 0;
        else ++n[S_BAD];
        if (n[S_COOL] > 0) --n[S_COOL], n[S_BAD] = 0;
        if (n[S_BAD] > c.sched_patience) {
            const double reduced = lr * c.factor, next = reduced > c.min_lr ? reduced : c.min_lr;
            if (lr - next > c.eps) lr = next;
            n[S_COOL] = c.sched_cooldown, n[S_BAD] = 0;
        }
    }
    // check_convergence(loss)
    bool done = false;
    float* w = f + S_WINDOW;
    if (cur <= c.abs_tol) {
        done = true;
    } else if (n[S_WLEN] < c.patience) {
        w[n[S_WLEN]++] = total;
    } else if (fabs(cur - (double)w[0]) < c.rel_tol) {
        done = true;
    } else {
        for (int k = 1; k < c.patience; ++k) w[k - 1] = w[k];
        w[c.patience - 1] = total;
    }
    f[S_TOTAL] = total, f[S_UP] = cost[0], f[S_LAT] = cost[1];
    n[S_DONE] = done ? 1 : 0;
}

// One block per image: word k of the image's records is summed by kChains chains (record t goes to chain t % kChains), the
// chains are added in order, all in float64; thread 0 then forms the eight numbers and either writes them (out) or moves the
// image's state by one step and leaves the pose of the new state (state; rpv then points into it, hence no __restrict__).
__global__ __launch_bounds__(kBlock) void param_opt_finish_kernel(const float* __restrict__ rec, int tiles, int H, int W,
                                                                  const float* rpv, int rpv_stride, float* pose,
                                                                  float* out, uint32_t* state, const ParamOptCfg cfg, int* n_done) {
    __shared__ double part[kChains][kRecWords];
    const int b = blockIdx.x, k = threadIdx.x & (kRecWords - 1), chain = threadIdx.x / kRecWords;
    uint32_t* s = state ? state + (size_t)b * kStateWords : nullptr;
    if (s && s[S_DONE]) return;               // (uniform)
    part[chain][k] = chain_sum<kChains>(rec + (size_t)b * tiles * kRecWords + k, kRecWords, tiles, chain);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum[kRecWords];
    for (int j = 0; j < kRecWords; ++j) sum[j] = column_sum(part, j);
    float* P = pose + (size_t)b * kPoseWords;
    const double inv = 1.0 / ((double)H * W), half = 0.5 * (double)rpv[(size_t)b * rpv_stride + 2], sh = sin(half);
    const double dfdv = -0.25 * H / (sh * sh), ifx = P[3], gc = P[2];
    const float cost[kRecWords] = {(float)(sum[0] * inv), (float)(sum[1] * inv), (float)(sum[2] * inv), (float)(sum[3] * inv),
                                   (float)(sum[4] * gc * ifx * dfdv * inv), (float)(sum[5] * inv), (float)(sum[6] * inv),
                                   (float)(-sum[7] * ifx * dfdv * inv)};
    if (out)
        for (int j = 0; j < kRecWords; ++j) out[(size_t)b * kRecWords + j] = cost[j];
    if (s) {
        param_opt_update(s, cost, cfg);
        write_pose(reinterpret_cast<const float*>(s), H, W, P);
        if (s[S_DONE]) atomicAdd(n_done, 1);
    }
}

// gclm_param_opt_cost: the pose records of given parameters, one lane per image.
__global__ void param_opt_pose_kernel(const float* __restrict__ rpv, int B, int H, int W, float* pose) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) write_pose(rpv + (size_t)b * 3, H, W, pose + (size_t)b * kPoseWords);
}

// gclm_param_opt_step: one lane per image.
__global__ void param_opt_step_kernel(uint32_t* state, const float* __restrict__ cost, int B, const ParamOptCfg cfg) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    uint32_t* s = state + (size_t)b * kStateWords;
    if (!s[S_DONE]) param_opt_update(s, cost + (size_t)b * kRecWords, cfg);
}

// The fresh state record of every image, from the caller's (r, p, v) or from the reference's _get_init_params: roll =
// -atan2(up_x, -up_y) and pitch = latitude at pixel (int(H / 2), int(W / 2)), vfov = |lat[0, W / 2] - lat[H - 1, W / 2]| held
// to [20, 120] degrees -- and then, as the reference does, read back from the objects it builds of them: roll and pitch
// through Gravity.from_rp(...).roll / .pitch (roll = asin(-g_x / (sqrt(1 - g_z^2) + 1e-4)), mirrored where g_y >= 0),
// vfov through the focal length.  float64 from the float32 pixels, rounded once.
__global__ void param_opt_init_kernel(const float* __restrict__ up, const float* __restrict__ lat, const float* __restrict__ init,
                                      int B, int H, int W, double lr, uint32_t* state, float* pose, int* n_done) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) *n_done = 0;
    if (b >= B) return;
    uint32_t* s = state + (size_t)b * kStateWords;
    float* f = reinterpret_cast<float*>(s);
    for (int k = 0; k < kStateWords; ++k) s[k] = 0u;
    if (init) {
        for (int k = 0; k < 3; ++k) f[S_RPV + k] = init[(size_t)b * 3 + k];
    } else {
        const size_t hw = (size_t)H * W, c = (size_t)(H / 2) * W + W / 2;
        const float* u = up + (size_t)b * 2 * hw;
        const float* l = lat + (size_t)b * hw;
        const float r0 = -atan2f(u[c], -u[hw + c]), p0 = l[c];
        float v0 = fabsf(l[W / 2] - l[(size_t)(H - 1) * W + W / 2]);
        const float vlo = (float)(20.0 / 180.0 * 3.14159265358979323846), vhi = (float)(120.0 / 180.0 * 3.14159265358979323846);
        v0 = v0 < vlo ? vlo : (v0 > vhi ? vhi : v0);              // (a NaN stays NaN)
        const double gx = -sin((double)r0) * cos((double)p0), gy = -cos((double)r0) * cos((double)p0), gz = sin((double)p0);
        const double gn = sqrt(gx * gx + gy * gy + gz * gz), x = gx / gn, yy = gy / gn, z = gz / gn;
        double roll = asin(-x / (sqrt(1.0 - z * z) + 1e-4));
        if (!(yy < 0.0)) roll = -roll - 3.14159265358979323846 * (x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0));
        const double focal = 0.5 * H / tan(0.5 * (double)v0);
        f[S_RPV] = (float)roll, f[S_RPV + 1] = (float)asin(z), f[S_RPV + 2] = (float)(2.0 * atan(H / (2.0 * focal)));
    }
    for (int k = 0; k < 3; ++k) f[S_INIT + k] = f[S_RPV + k];
    *reinterpret_cast<double*>(s + S_LR) = lr;
    f[S_BEST] = __builtin_inff();
    write_pose(f, H, W, pose + (size_t)b * kPoseWords);
}

// d_rpv and d_info of the finished loop.
__global__ void param_opt_result_kernel(const uint32_t* __restrict__ state, int B, float* rpv, float* info) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t* s = state + (size_t)b * kStateWords;
    const float* f = reinterpret_cast<const float*>(s);
    for (int k = 0; k < 3; ++k) rpv[(size_t)b * 3 + k] = f[S_RPV + k];
    float* o = info + (size_t)b * kInfoWords;
    o[0] = (float)(int32_t)s[S_STEPS], o[1] = (float)(int32_t)s[S_DONE], o[2] = f[S_TOTAL], o[3] = f[S_UP], o[4] = f[S_LAT];
    o[5] = (float)*reinterpret_cast<const double*>(s + S_LR);
    for (int k = 0; k < 3; ++k) o[6 + k] = f[S_INIT + k];
    for (int k = 9; k < kInfoWords; ++k) o[k] = 0.f;
}

ParamOptCfg device_config(const gclm_param_opt_config& c) {
    return {c.patience, c.use_scheduler, c.sched_patience, c.sched_cooldown, c.lr, c.abs_tol, c.rel_tol, c.lamb, c.sched_factor,
            c.sched_threshold, c.sched_min_lr, c.sched_eps};
}

// Where the parts of a workspace lie: tile records, pose records, state records, the count of converged images.
struct Workspace {
    float *rec, *pose;
    uint32_t* state;
    int* n_done;
};

size_t record_bytes(int B, int H, int W) { return tile_record_bytes(B, H, W, kRecWords, sizeof(float)); }

Workspace carve(void* workspace, int B, int H, int W) {
    char* p = static_cast<char*>(workspace);
    Workspace w;
    w.rec = reinterpret_cast<float*>(p);
    p += record_bytes(B, H, W);
    w.pose = reinterpret_cast<float*>(p);
    p += (size_t)B * kPoseWords * sizeof(float);
    w.state = reinterpret_cast<uint32_t*>(p);
    p += (size_t)B * kStateWords * sizeof(uint32_t);
    w.n_done = reinterpret_cast<int*>(p);
    return w;
}

hipError_t launch_pass(const float* up, const float* lat, const float* pose, const int32_t* done, float* rec, int B, int H, int W,
                       int px, hipStream_t st) {
    const PassArgs a{up, lat, pose, done, rec, H, W, tile_columns(W, px)};
    const auto kernel = with_pixels_per_lane(px, [](auto p) { return param_opt_pass_kernel<decltype(p)::value>; });
    hipLaunchKernelGGL(kernel, dim3(tile_count(H, W, px), B), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace

size_t param_opt_workspace(int B, int H, int W) {
    if (!call_sizes_fit(B, H, W) || H < 2 || W < 2) return 0;
    return record_bytes(B, H, W) + (size_t)B * (kPoseWords * sizeof(float) + kStateWords * sizeof(uint32_t)) + 16;
}

hipError_t launch_param_opt_cost(const float* up, const float* lat, const float* rpv, int B, int H, int W, void* workspace,
                                 float* out, hipStream_t st) {
    const Workspace w = carve(workspace, B, H, W);
    const int px = pixels_per_lane(W, {up, lat});
    hipLaunchKernelGGL(param_opt_pose_kernel, dim3((B + 63) / 64), dim3(64), 0, st, rpv, B, H, W, w.pose);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_pass(up, lat, w.pose, nullptr, w.rec, B, H, W, px, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(param_opt_finish_kernel, dim3(B), dim3(kBlock), 0, st, w.rec, tile_count(H, W, px), H, W, rpv, 3, w.pose, out,
                       (uint32_t*)nullptr, ParamOptCfg{}, (int*)nullptr);
    return hipGetLastError();
}

hipError_t launch_param_opt_step(void* state, const float* cost, int B, const gclm_param_opt_config& cfg, hipStream_t st) {
    hipLaunchKernelGGL(param_opt_step_kernel, dim3((B + 63) / 64), dim3(64), 0, st, static_cast<uint32_t*>(state), cost, B,
                       device_config(cfg));
    return hipGetLastError();
}

hipError_t launch_param_opt(const float* up, const float* lat, const float* init, int B, int H, int W,
                            const gclm_param_opt_config& cfg, void* workspace, float* rpv, float* info, hipStream_t st) {
    const Workspace w = carve(workspace, B, H, W);
    const int px = pixels_per_lane(W, {up, lat}), tiles = tile_count(H, W, px);
    const ParamOptCfg c = device_config(cfg);
    hipLaunchKernelGGL(param_opt_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, up, lat, init, B, H, W, cfg.lr, w.state, w.pose,
                       w.n_done);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int32_t* done = reinterpret_cast<const int32_t*>(w.state) + S_DONE;
    for (int step = 1; step <= cfg.max_steps; ++step) {
        if ((e = launch_pass(up, lat, w.pose, done, w.rec, B, H, W, px, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(param_opt_finish_kernel, dim3(B), dim3(kBlock), 0, st, w.rec, tiles, H, W,
                           reinterpret_cast<const float*>(w.state), kStateWords, w.pose, (float*)nullptr, w.state, c, w.n_done);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (cfg.poll_every > 0 && step % cfg.poll_every == 0 && step < cfg.max_steps) {
            int n_done = 0;                   // the sync the caller asked for
            if ((e = hipMemcpyAsync(&n_done, w.n_done, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
            if (n_done >= B) break;
        }
    }
    hipLaunchKernelGGL(param_opt_result_kernel, dim3((B + 63) / 64), dim3(64), 0, st, w.state, B, rpv, info);
    return hipGetLastError();
}

}  // namespace gclm
