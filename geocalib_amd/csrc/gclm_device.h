// gclm_device.h -- per-image device logic shared by the update kernels (gclm_update.hip), the prologue of the
// one-launch-per-step sweep for single images (gclm_pass.hip: fused_step_kernel) and the stage kernels.  gfx950 only.
#pragma once
#include "gclm_internal.h"

namespace gclm {
namespace dev {

// The per-image arithmetic below is compiled into several kernels of two translation units (update_kernel,
// shared_step_kernel, fused_step_kernel ...) that must produce the SAME BITS (the one-launch-per-step path is checked
// bit for bit against the two-launch path).  With contraction on, the backend decides per inlining context which
// a * b + c becomes an fma, so contraction is switched off for this header: every operation here is an IEEE operation
// (the fmas that are wanted are written as fmaf).  Restored at the end of the file -- the per-pixel code keeps it.
// (Needs -ffp-contract=fast-honor-pragmas: plain `fast` ignores this pragma.)
#pragma clang fp contract(off)

constexpr float kPi = 3.14159265358979323846f;

struct V3 { float x, y, z; };

// ---------------------------------------------------------------- gravity / manifold (device)

// Gravity.roll / pitch (gravity.py:63-81)
__device__ inline float grav_roll(V3 g) {
    const float roll = asinf(-g.x / (sqrtf(1.0f - g.z * g.z) + 1e-4f));
    const float sgn = (g.x > 0.f) ? 1.f : ((g.x < 0.f) ? -1.f : 0.f);
    return g.y < 0.f ? roll : -roll - kPi * sgn;
}
__device__ inline float grav_pitch(V3 g) { return asinf(g.z); }

// Gravity.J_rp (gravity.py:69-101): T[i][k], k = roll, pitch
__device__ inline void tangent_rp(V3 g, float (&T)[3][2]) {
    const float r = grav_roll(g), p = grav_pitch(g);
    float sr, cr, sp, cp;
    sincosf(r, &sr, &cr);
    sincosf(p, &sp, &cp);
    T[0][0] = -cr * cp; T[1][0] = sr * cp; T[2][0] = 0.f;
    T[0][1] = sr * sp;  T[1][1] = cr * sp; T[2][1] = cp;
}

// SphericalManifold.householder_vector (misc.py:182-209), pivot = last component
__device__ inline void householder(V3 x, float (&v)[3], float& beta) {
    float sigma = x.x * x.x + x.y * x.y;
    const float norm = sqrtf(sigma + x.z * x.z);
    if (sigma < 1e-7f) sigma += 1e-7f;
    const float vpiv = x.z < 0.f ? x.z - norm : -sigma / (x.z + norm);
    beta = 2.f * vpiv * vpiv / (sigma + vpiv * vpiv);
    v[0] = x.x / vpiv; v[1] = x.y / vpiv; v[2] = 1.f;
}

// SphericalManifold.J_plus (misc.py:226-231)
__device__ inline void tangent_sphere(V3 g, float (&T)[3][2]) {
    float v[3], beta;
    householder(g, v, beta);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k) T[i][k] = -beta * v[i] * v[k] + (i == k ? 1.f : 0.f);
}

__device__ inline V3 normalize3(V3 g) {
    const float n = fmaxf(sqrtf(g.x * g.x + g.y * g.y + g.z * g.z), 1e-12f);
    return {g.x / n, g.y / n, g.z / n};
}

__device__ inline V3 from_rp(float roll, float pitch) {   // gravity.py:31-40
    float sr, cr, sp, cp;
    sincosf(roll, &sr, &cr);
    sincosf(pitch, &sp, &cp);
    return normalize3({-sr * cp, -cr * cp, sp});
}

// Gravity.update (gravity.py:112-119) / SphericalManifold.plus (misc.py:234-259), in two halves: what depends on the OLD
// gravity only (its norm and Householder vector) and what needs the step.  The one-launch-per-step kernel computes the
// first half on another wave while the normal equations are still being solved (same operations, same bits).
struct GravPre {
    float v[3], beta, nx;
};
__device__ inline void grav_update_pre(V3 g, GravPre& p) {
    p.nx = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
    householder(g, p.v, p.beta);
}
__device__ inline V3 grav_update_post(const GravPre& p, float d0, float d1) {
    const float eps = 1e-7f;
    const float nd = sqrtf(d0 * d0 + d1 * d1);
    const float nd_ = nd < eps ? nd + eps : nd;
    const float sinc = nd < eps ? 1.f : sinf(nd_) / nd_;
    const float e[3] = {sinc * d0, sinc * d1, cosf(nd)};
    const float bd = p.beta * (p.v[0] * e[0] + p.v[1] * e[1] + p.v[2] * e[2]);
    return normalize3({p.nx * (e[0] - p.v[0] * bd), p.nx * (e[1] - p.v[1] * bd), p.nx * (e[2] - p.v[2] * bd)});
}
__device__ inline V3 grav_update(V3 g, float d0, float d1, bool spherical) {
    if (!spherical) return from_rp(grav_roll(g) + d0, grav_pitch(g) + d1);
    GravPre p;
    grav_update_pre(g, p);
    return grav_update_post(p, d0, d1);
}

// BaseCamera.update_focal (camera.py:136-152): clamp to fov in [5, 150] deg of the image HEIGHT,
// fx rebuilt from fy by the old ratio.
__device__ inline void update_focal(State& s, float delta, bool as_log) {
    const float fy = as_log ? expf(logf(s.fy) + delta) : s.fy + delta;
    // fov2focal(ones * deg2rad(150), h), fov2focal(ones * deg2rad(5), h) in float32 as the reference evaluates them: deg2rad
    // of a Python number is a double, rounded to float32 by the product; tan of its half in float32.  (tan of the
    // float32-ARITHMETIC 5 / 180 * pi is 0.043660946f, one ulp up: the bound came out one ulp low at 93 % of all heights.)
    const float min_f = s.h * 0.5f / 3.7320504f;
    const float max_f = s.h * 0.5f / 0.043660942f;
    const float fyc = fminf(fmaxf(fy, min_f), max_f);
    s.fx = fyc * s.fx / s.fy;
    s.fy = fyc;
}

// SimpleRadial.update_dist (camera.py:599-604); slot 7 shadows k1 for one-parameter models
__device__ inline void update_dist(State& s, int camera_model, float d1, float d2) {
    // range (-0.7, 0.7), simple_divisional (-3, 3)  (camera.py:599, 700, 817)
    const float hi = camera_model == GCLM_SIMPLE_DIVISIONAL ? 3.0f : 0.7f;
    s.k1 = fminf(fmaxf(s.k1 + d1, -hi), hi);
    s.k2 = fminf(fmaxf(s.k2 + (camera_model == GCLM_RADIAL ? d2 : d1), -hi), hi);
}

// The parameter block of a state, in two halves: the tangent basis of its gravity (the long chain: a Householder vector,
// or asin / sincos for the (roll, pitch) form) and the rest (two reciprocals).  build_pblock = fill_pblock(tangent).
__device__ inline void pblock_tangent(V3 g, bool spherical, float (&T)[3][2]) {
    if (spherical) tangent_sphere(g, T); else tangent_rp(g, T);
}
__device__ inline void fill_pblock(const State& s, const float (&T)[3][2], float ifx, float ify, bool log_focal, PBlock& p) {
    p.ifx = ifx; p.ify = ify; p.cx = s.cx; p.cy = s.cy;
    p.ga = s.gx; p.gb = s.gy; p.gc = s.gz; p.k1 = s.k1;
    p.T00 = T[0][0]; p.T01 = T[0][1]; p.T10 = T[1][0]; p.T11 = T[1][1]; p.T20 = T[2][0]; p.T21 = T[2][1];
    p.wfx = log_focal ? 1.0f : ifx;
    p.wfy = log_focal ? 1.0f : ify;
    p.k2 = s.k2; p.pad0 = p.pad1 = p.pad2 = 0.f;
}
__device__ inline void build_pblock(const State& s, bool spherical, bool log_focal, PBlock& p) {
    float T[3][2];
    pblock_tangent({s.gx, s.gy, s.gz}, spherical, T);
    fill_pblock(s, T, 1.0f / s.fx, 1.0f / s.fy, log_focal, p);
}

// A camera row (GCLM_CAM_STRIDE floats, BaseCamera._data) plus a gravity vector (normalised here) as a State, and back:
// every kernel that takes or hands out (cam, grav) goes through these two.  The optimiser's own fields are left zero.
static_assert(GCLM_CAM_STRIDE == 8, "w h fx fy cx cy k1 k2");
__device__ inline State state_from_params(const float* cm, const float* grav) {
    State s{};
    s.w = cm[0]; s.h = cm[1]; s.fx = cm[2]; s.fy = cm[3]; s.cx = cm[4]; s.cy = cm[5]; s.k1 = cm[6]; s.k2 = cm[7];
    const V3 g = normalize3({grav[0], grav[1], grav[2]});
    s.gx = g.x; s.gy = g.y; s.gz = g.z;
    return s;
}
__device__ inline void params_from_state(const State& s, float* cm, float* grav) {
    cm[0] = s.w; cm[1] = s.h; cm[2] = s.fx; cm[3] = s.fy; cm[4] = s.cx; cm[5] = s.cy; cm[6] = s.k1; cm[7] = s.k2;
    grav[0] = s.gx; grav[1] = s.gy; grav[2] = s.gz;
}

// The initial estimate of image b: the caller's (gclm_solve) or get_trivial_estimation / siclib's heuristic from the priors
// (gclm_calibrate).  init_kernel runs it once per image; the one-launch-per-step kernel runs it in the prologue of its
// first launch instead (every workgroup of the image, same bits), which saves a single-image solve the init launch.
__device__ inline State init_state(const SolveCtx& c, const InitArgs& ia, int b) {
    State s;
    if (ia.cam) {       // caller-provided initial estimate
        s = state_from_params(ia.cam + (size_t)b * GCLM_CAM_STRIDE, ia.grav + b * 3);
    } else {            // get_trivial_estimation (lm_optimizer.py:20-58) + BaseCamera.from_dict (camera.py:49-93)
        const float h = (float)c.H, w = (float)c.W;
        const float focal = ia.prior_focal ? ia.prior_focal[b] : 0.7f * fmaxf(h, w);
        const float vfov = 2.0f * atanf(h / (2.0f * focal));           // focal2fov
        const float f = h / 2.0f / tanf(vfov / 2.0f);                   // fov2focal
        s.w = w; s.h = h; s.fy = f; s.cx = w / 2.0f; s.cy = h / 2.0f;
        s.fx = ia.scales ? f * ia.scales[0] / ia.scales[1] : f;
        s.k1 = s.k2 = 0.f;
        if (ia.prior_dist) {
            const int nd = ia.prior_dist_cols;
            s.k1 = ia.prior_dist[(size_t)b * nd];
            if (nd > 1) s.k2 = ia.prior_dist[(size_t)b * nd + 1];
        }
        V3 g{-0.0f, -1.0f, 0.0f};                                     // Gravity.from_rp(0, 0)
        if (c.cfg.heuristic_init && ia.up) {
            // get_heuristic_estimation (siclib/models/optimization/utils.py:27-82): roll = angle of the up
            // vector at the image centre, pitch = latitude at the centre, vfov = |lat(top) - lat(bottom)|
            // on the central column, all clamped; priors still win below
            const size_t N = (size_t)c.H * c.W;
            const int yc = c.H / 2, xc = c.W / 2;
            const float* up = ia.up + (size_t)b * 2 * N;
            const float* lat = ia.lat + (size_t)b * N;
            const float d45 = 45.0f / 180.0f * kPi;
            float roll = -atan2f(up[(size_t)yc * c.W + xc], -up[N + (size_t)yc * c.W + xc]);
            roll = fminf(fmaxf(roll, -d45), d45);
            const float pitch = fminf(fmaxf(lat[(size_t)yc * c.W + xc], -d45), d45);
            float vfov_h = fabsf(lat[xc] - lat[(size_t)(c.H - 1) * c.W + xc]);
            vfov_h = fminf(fmaxf(vfov_h, 20.0f / 180.0f * kPi), 120.0f / 180.0f * kPi);
            if (!ia.prior_focal) {
                const float fh = h / 2.0f / tanf(vfov_h / 2.0f);
                s.fy = fh;
                s.fx = ia.scales ? fh * ia.scales[0] / ia.scales[1] : fh;
            }
            g = from_rp(roll, pitch);
        }
        if (ia.prior_gravity) g = normalize3({ia.prior_gravity[b * 3], ia.prior_gravity[b * 3 + 1], ia.prior_gravity[b * 3 + 2]});
        s.gx = g.x; s.gy = g.y; s.gz = g.z;
    }
    s.lambda = c.cfg.lambda0; s.prev_cost = 0.f; s.fails = 0.f; s.init_cu = s.init_cl = 0.f;
    return s;
}

// ---------------------------------------------------------------- small dense algebra
// Everything here has compile-time sizes and fully unrolled loops so that the tiny matrices live in
// registers: a dynamically indexed local array is placed in scratch memory on gfx950 and made the
// first generic version of the update kernel 2.5x slower (42 us vs 17 us per launch at B = 1024).

// In-place Cholesky solve of an N x N SPD system (fp32 like torch.linalg.cholesky on fp32).
template <int N>
__device__ inline bool chol_solve(float (&A)[N][N], float (&b)[N]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        float s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= A[j][k] * A[j][k];
        ok = ok && (s > 0.f);
        const float l = sqrtf(s);
        A[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            float t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= A[i][k] * A[j][k];
            A[i][j] = t / l;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float t = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= A[i][k] * b[k];
        b[i] = t / A[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        float t = b[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) t -= A[k][i] * b[k];
        b[i] = t / A[i][i];
    }
    return ok;
}

// Symmetric PM x PM system (PM = 4 or 5 full columns d1,d2,f,k1[,k2]) out of an accumulator record.
template <int PM>
__device__ inline void unpack_system(const float* acc, float (&Hm)[PM][PM], float (&G)[PM]) {
#pragma unroll
    for (int i = 0; i < PM; ++i) {
        G[i] = acc[A_G0 + i];
#pragma unroll
        for (int j = i; j < PM; ++j) Hm[i][j] = Hm[j][i] = acc[acc_h(PM, i, j)];
    }
}

// Which of the PM full columns are free (calculate_gradient_and_hessian, lm_optimizer.py:335-344).  The
// system is solved at its full size with the fixed columns replaced by identity rows -- arithmetically the
// reference's sub-matrix solve (the masked entries only ever contribute exact zeros), without dynamic indexing.
template <int PM>
__device__ inline void active_columns(const gclm_config& cfg, bool (&act)[PM]) {
    const int nd = num_dist_params(cfg.camera_model);
#pragma unroll
    for (int k = 0; k < PM; ++k)
        act[k] = k < 2 ? cfg.estimate_gravity != 0 : (k == 2 ? cfg.estimate_focal != 0 : k - 3 < nd);
}

// The steps of update_estimate (lm_optimizer.py:518-549) out of the full-size solution, reproducing the python
// index arithmetic of :223-235: dist_delta_dims start at focal_delta_dims[-1] + 1, which is 0 when the focal is a
// prior -- i.e. the distortion then takes the GRAVITY steps (reference quirk, kept).
template <int PM>
__device__ inline void split_delta(const gclm_config& cfg, const float (&d)[PM], float& dg0, float& dg1, float& df,
                                   float& dk1, float& dk2) {
    const bool eg = cfg.estimate_gravity != 0, ef = cfg.estimate_focal != 0;
    dg0 = eg ? d[0] : 0.f;
    dg1 = eg ? d[1] : 0.f;
    df = ef ? d[2] : 0.f;
    const float d4 = PM > 4 ? d[PM - 1] : 0.f;
    dk1 = (ef || !eg) ? d[3] : d[0];
    dk2 = (ef || !eg) ? d4 : d[1];
}

// sum(c.mean(-1) for c in costs.values()) (lm_optimizer.py:584,610), float32
__device__ inline float total_cost(const float* acc, float invN, bool has_up, float& cu, float& cl) {
    cu = acc[A_CU] * invN;
    cl = acc[A_CL] * invN;
    return has_up ? cu + cl : cl;
}

// update_lambda (lm_optimizer.py:95-106) of one image whose new cost is `total`
__device__ inline void lambda_rule(float total, State& s) {
    const float nl = s.lambda * (total > s.prev_cost ? 10.f : 0.1f);
    s.lambda = fminf(fmaxf(nl, 1e-6f), 1e2f);
}

// lambda rule + "allclose" test of one image (lm_optimizer.py:95-106, :90-92, :612-627): returns whether the cost
// still MOVED at this step (always false at step 0, where nothing is compared); the caller counts it.
__device__ inline bool cost_rules(const gclm_config& cfg, int step, float total, State& s, bool update_lambda) {
    bool moved = false;
    if (step > 0) {
        if (update_lambda) lambda_rule(total, s);
        // torch.allclose evaluates |new - prev| <= atol + |rtol * prev| in the tensors' dtype (float32: the scalar tolerances
        // do not promote; ATen isclose) -- so does this (rounds 1-3 used double: same decision unless the difference sits
        // within 1e-15 of the threshold, but it was a deviation nobody had written down)
        const float diff = fabsf(total - s.prev_cost);
        moved = !(diff <= cfg.atol + fabsf(cfg.rtol * s.prev_cost));
    }
    s.prev_cost = total;
    return moved;
}

// ... and the batch-global bookkeeping on top of it: every image whose cost moved counts into notclose[step]
__device__ inline void cost_bookkeeping(const gclm_config& cfg, Ctrl* ctrl, int step, float total,
                                        State& s, bool update_lambda) {
    if (cost_rules(cfg, step, total, s, update_lambda)) atomicAdd(&ctrl->notclose[step], 1);
}

// One LM step of one image from its reduced accumulator record, as pure arithmetic on (s, acc), in stages:
//   lm_solve          lambda rule + allclose test, damped normal equations over the estimated columns -> the steps `dl`
//                     (updates s.lambda / prev_cost / fails / init_*; returns whether the cost moved)
//   lm_apply_gravity / lm_apply_focal / lm_apply_dist    manifold / focal / distortion update: independent of each other
// lm_step runs them in sequence on one thread (update_kernel); the one-launch-per-step kernel runs the three updates on
// three waves at once (fused_step_kernel).  `s` is the state at `step` on entry and the state at step + 1 on return.
struct StepDelta {
    float dg0, dg1, df, dk1, dk2;
};
// (`d`: the full-size solution over the columns (d1, d2, f, k1[, k2]), zero in fixed columns and after a failed step --
//  what the step record of gclm_solve_recorded keeps;
//  `prior_mean_cost`: null, or the soft priors' cost / N at this state (add_soft_priors), which joins the compared cost)
template <int PM>
__device__ inline bool lm_solve(const gclm_config& cfg, int H, int W, int step, State& s, const float (&acc)[kNAccMax],
                                StepDelta& dl, float (&d)[PM], const float* prior_mean_cost = nullptr) {
    const float invN = 1.0f / (float)((size_t)H * W);
    float cu, cl;
    float total = total_cost(acc, invN, true, cu, cl);   // A_CU is 0 without an up field
    if (prior_mean_cost) total = total + *prior_mean_cost;
    if (step == 0) { s.init_cu = cu; s.init_cl = cl; }     // infos["initial_*"] (:585-588)
    const bool moved = cost_rules(cfg, step, total, s, !cfg.fix_lambda);

    // damped normal equations over the estimated columns (lm_optimizer.py:109-137)
    float A[PM][PM];
    bool act[PM];
    unpack_system<PM>(acc, A, d);
    active_columns<PM>(cfg, act);
#pragma unroll
    for (int i = 0; i < PM; ++i) {
#pragma unroll
        for (int j = 0; j < PM; ++j)
            if (!(act[i] && act[j])) A[i][j] = i == j ? 1.f : 0.f;
        if (act[i]) A[i][i] += fmaxf(A[i][i] * s.lambda, 1e-6f); else d[i] = 0.f;
    }
    bool ok = chol_solve<PM>(A, d);
#pragma unroll
    for (int i = 0; i < PM; ++i) ok = ok && fabsf(d[i]) <= 3.0e38f;      // a NaN / inf step (NaN gradient) is a failed step too
    if (!ok) {
#pragma unroll
        for (int i = 0; i < PM; ++i) d[i] = 0.f;     // zero step for THIS image (reference: whole batch)
        s.fails += 1.f;
    }
    split_delta<PM>(cfg, d, dl.dg0, dl.dg1, dl.df, dl.dk1, dl.dk2);
    return moved;
}
template <int PM>
__device__ inline bool lm_solve(const gclm_config& cfg, int H, int W, int step, State& s, const float (&acc)[kNAccMax],
                                StepDelta& dl) {
    float d[PM];
    return lm_solve<PM>(cfg, H, W, step, s, acc, dl, d);
}
__device__ inline void lm_apply_gravity(const gclm_config& cfg, State& s, const StepDelta& dl) {
    const V3 g = grav_update({s.gx, s.gy, s.gz}, dl.dg0, dl.dg1, cfg.use_spherical_manifold != 0);
    s.gx = g.x; s.gy = g.y; s.gz = g.z;
}
__device__ inline void lm_apply_focal(const gclm_config& cfg, State& s, const StepDelta& dl) {
    update_focal(s, dl.df, cfg.use_log_focal != 0);
}
__device__ inline void lm_apply_dist(const gclm_config& cfg, State& s, const StepDelta& dl) {
    if (cfg.camera_model != GCLM_PINHOLE && cfg.estimate_dist) update_dist(s, cfg.camera_model, dl.dk1, dl.dk2);
}
template <int PM>
__device__ inline bool lm_step(const gclm_config& cfg, int H, int W, int step, State& s, const float (&acc)[kNAccMax],
                               float (&d)[PM], const float* prior_mean_cost = nullptr) {
    StepDelta dl;
    const bool moved = lm_solve<PM>(cfg, H, W, step, s, acc, dl, d, prior_mean_cost);
    lm_apply_gravity(cfg, s, dl);
    lm_apply_focal(cfg, s, dl);
    lm_apply_dist(cfg, s, dl);
    return moved;
}
template <int PM>
__device__ inline bool lm_step(const gclm_config& cfg, int H, int W, int step, State& s, const float (&acc)[kNAccMax]) {
    float d[PM];
    return lm_step<PM>(cfg, H, W, step, s, acc, d);
}

// Soft priors (gclm_calibrate_soft): a prior given with its standard deviation is one more observation of image b, in the
// sum convention of the sweep's record (cost sum rho, H = sum w J^T J, G = sum w J^T r, r = target - model), at state s:
//   focal    on the log-focal column 2: w = (f0 / sigma_f)^2, r = log f0 - log fy;  G[2] += w r, H[2][2] += w, cost w r^2
//            (r as log(f0 / fy): the difference of two float32 logarithms of ~3 would carry 1e-5 of a residual of 0.03)
//   gravity  g0 = normalize(prior), w = 1 / sigma_g^2, r = g0 - g, T the 3x2 tangent basis of columns 0 and 1 (the sweep's:
//            pblock_tangent);  G[0:2] += w T^T r, H[0:2,0:2] += w T^T T, cost w |r|^2
// added to the image's REDUCED record `acc`; the cost is returned (to be divided by N like the data costs) and not folded
// into A_CU / A_CL, which stay the data's.  `final_form`: the record is the uncertainty sweep's, over (roll, pitch, plain
// focal): only the information is added, T = tangent_rp and 1 / sigma_f^2 on the focal diagonal -- times fy^2 where the sweep
// ran the log-focal form that finalize_kernel rescales by 1 / fy (`iso_final`).  The cost is that of the LM form either way.
// A sigma that is not finite and positive (or a prior that cannot be used: non-positive focal, NaN) leaves its term out and
// sets `bad`; the caller counts a failed step.  Weights that underflow add exact zeros: sigma = 1e30 is the free solve's bits.
struct PriorTerms {
    float cost;
    bool bad;
};
__device__ inline bool finite_positive(float v) { return v > 0.f && v <= 3.0e38f; }
template <int PM>
__device__ inline PriorTerms add_soft_priors(const gclm_config& cfg, const SoftPrior& sp, int b, const State& s, bool final_form,
                                             bool iso_final, float (&acc)[kNAccMax]) {
    PriorTerms out{0.f, false};
    if (sp.focal_sigma) {
        const float f0 = sp.focal[b], sg = sp.focal_sigma[b];
        if (finite_positive(sg) && finite_positive(f0)) {
            const float q = f0 / sg, w = q * q, r = logf(f0 / s.fy);
            out.cost += w * r * r;
            if (!final_form) {
                acc[A_G0 + 2] += w * r;
                acc[acc_h(PM, 2, 2)] += w;
            } else {
                const float qf = (iso_final ? s.fy : 1.0f) / sg;
                acc[acc_h(PM, 2, 2)] += qf * qf;
            }
        } else {
            out.bad = true;
        }
    }
    if (sp.gravity_sigma) {
        const float sg = sp.gravity_sigma[b];
        const V3 g0 = normalize3({sp.gravity[b * 3], sp.gravity[b * 3 + 1], sp.gravity[b * 3 + 2]});
        const float n0 = g0.x * g0.x + g0.y * g0.y + g0.z * g0.z;
        if (finite_positive(sg) && n0 > 0.5f && n0 < 2.0f) {        // (a zero or NaN prior vector does not normalise)
            const float is = 1.0f / sg, w = is * is;
            const float r[3] = {g0.x - s.gx, g0.y - s.gy, g0.z - s.gz};
            float T[3][2];
            if (final_form) tangent_rp({s.gx, s.gy, s.gz}, T);
            else pblock_tangent({s.gx, s.gy, s.gz}, cfg.use_spherical_manifold != 0, T);
            out.cost += w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            if (!final_form) {
                acc[A_G0 + 0] += w * (T[0][0] * r[0] + T[1][0] * r[1] + T[2][0] * r[2]);
                acc[A_G0 + 1] += w * (T[0][1] * r[0] + T[1][1] * r[1] + T[2][1] * r[2]);
            }
            acc[acc_h(PM, 0, 0)] += w * (T[0][0] * T[0][0] + T[1][0] * T[1][0] + T[2][0] * T[2][0]);
            acc[acc_h(PM, 0, 1)] += w * (T[0][0] * T[0][1] + T[1][0] * T[1][1] + T[2][0] * T[2][1]);
            acc[acc_h(PM, 1, 1)] += w * (T[0][1] * T[0][1] + T[1][1] * T[1][1] + T[2][1] * T[2][1]);
        } else {
            out.bad = true;
        }
    }
    return out;
}
// The cost the damping rule and the early stop compare, with soft priors: (up + latitude) + prior / N, each operation
// rounded to float32 (here, where nothing contracts), so that infos["final_cost"] is that float32 sum of its three infos.
__device__ inline float prior_mean(float prior_cost, float invN) { return prior_cost * invN; }
__device__ inline float add_prior_mean(float data_total, float prior_cost_mean) { return data_total + prior_cost_mean; }

// The state after update `step` and its parameter block go into the OTHER half of the double buffers, for the next sweep.
__device__ inline void commit_state(const SolveCtx& c, int step, int b, const State& s) {
    c.state[(step + 1) & 1][b] = s;
    PBlock p;
    build_pblock(s, c.cfg.use_spherical_manifold != 0, c.cfg.use_log_focal != 0, p);
    c.pb[(step + 1) & 1][b] = p;
}

// infos["stop_at"] (lm_optimizer.py:575,619-620,638): the first step after which EVERY image's cost was "close", i.e. the
// first j in [1, num_steps) whose counter stayed 0, else num_steps (the counter of the last comparison cannot change the
// answer).  The counters of one batch may lie in the control blocks of `n` handles (gclm_merge_stop_at): their sum decides.
__device__ inline int first_quiet_step(const Ctrl* const* ctrl, int n, int num_steps) {
    for (int j = 1; j < num_steps; ++j) {
        int moved = 0;
        for (int p = 0; p < n; ++p) moved += ctrl[p]->notclose[j];
        if (moved == 0) return j;
    }
    return num_steps;
}
__device__ inline int first_quiet_step(const Ctrl* ctrl, int num_steps) { return first_quiet_step(&ctrl, 1, num_steps); }

// ---------------------------------------------------------------- reduction of the sweep's partial records
// A sweep leaves `nchunks` records of `nacc` floats per image; slot i of an image's system is the sum of slot i over them.
// Blocks of 256 threads = kGroups groups x kSlots slots reduce them (the first nacc = 16 or 24 slots are live).
constexpr int kGroups = 8, kSlots = 32, kStripeMinChunks = 33;
// THE stripe rule.  Few records per image (large batches): one ascending walk per slot.  From kStripeMinChunks on (small
// batches of large images, where one walk is a latency chain of hundreds of dependent loads): group g walks stripe g, g + 8,
// ... and the eight stripe sums are combined in stripe order.  Everything that depends on the choice derives from here.
struct Stripe { bool on; int first, stride; };
__host__ __device__ inline bool records_striped(int nchunks) { return nchunks >= kStripeMinChunks; }
__device__ inline Stripe stripe_of(int nchunks, int grp) {
    const bool on = records_striped(nchunks);
    return Stripe{on, on ? grp : 0, on ? kGroups : 1};
}
// THE record sum: records first, first + stride, ... < nchunks of one slot (`p`: that slot of record 0), in ascending
// order, in double.  BATCH loads are in flight together (a clamped index and a select instead of a branch), so the 15
// records of a 640x480 image, or the 19 of a stripe of a single one, cost one memory round trip.  The padding adds +0.0 to a
// double that is never -0.0 (it starts at +0.0, and x + -x rounds to +0.0), so BATCH cannot change a bit: every caller gets
// the same sum of the same records.  `after_first_batch()` runs once the first batch has been ISSUED and before anything
// waits for it -- a caller's own independent loads queue up BEHIND the records (loads return in order) -- in every
// thread, so call this in uniform control flow and say who sums with `active` (first < nchunks: an image has a record).
template <int BATCH, typename Hook>
__device__ inline double sum_records(bool active, const float* p, int nacc, int first, int stride, int nchunks,
                                     Hook&& after_first_batch) {
    float v[BATCH];
    auto load = [&](int c0) {
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int c = c0 + j * stride;
            const float t = p[(size_t)min(c, nchunks - 1) * nacc];
            v[j] = c < nchunks ? t : 0.f;
        }
    };
    if (active) load(first);
    after_first_batch();
    double d = 0.0;
    if (active) {
#pragma unroll
        for (int j = 0; j < BATCH; ++j) d += v[j];
        for (int c0 = first + BATCH * stride; c0 < nchunks; c0 += BATCH * stride) {
            load(c0);
#pragma unroll
            for (int j = 0; j < BATCH; ++j) d += v[j];
        }
    }
    return d;
}
template <int BATCH>
__device__ inline double sum_records(bool active, const float* p, int nacc, int first, int stride, int nchunks) {
    return sum_records<BATCH>(active, p, nacc, first, stride, nchunks, [] {});
}
// The records of ONE image summed by the whole block, stripes or one walk by the rule above: the prologue of the
// one-launch-per-step kernel, which passes its first field loads as the hook.  Must be called by all threads of the block.
// The sums are valid in the threads of WAVE 0 on return (lane i of wave 0 sums slot i over the stripes, v_readlane hands
// the values to the whole wave): round 3 had every one of the 256 threads read all 8 x 24 doubles back from LDS -- 1 us of
// LDS bandwidth at the head of every launch of a single-image solve (device trace, profiles/archive/r04_latency_trace.log).
template <typename Hook>
__device__ inline void reduce_image_partials(const float* image_partials, int nchunks, int nacc, float (&acc)[kNAccMax],
                                             Hook&& after_first_batch) {
    __shared__ double sacc1[kGroups][kSlots + 1];
    const int grp = threadIdx.x / kSlots, slot = threadIdx.x % kSlots;
    const Stripe st = stripe_of(nchunks, grp);
    const bool active = slot < nacc && (st.on || grp == 0);
    const double sum = sum_records<32>(active, image_partials + slot, nacc, st.first, st.stride, nchunks, after_first_batch);
    if (active) sacc1[grp][slot] = sum;
    __syncthreads();
    if (threadIdx.x < 64) {                                            // wave 0 (wave-uniform)
        double d = 0.0;
        if ((int)threadIdx.x < nacc) {
            if (st.on) { for (int g = 0; g < kGroups; ++g) d += sacc1[g][threadIdx.x]; }
            else d = sacc1[0][threadIdx.x];
        }
        const int mine = __builtin_bit_cast(int, (float)d);            // 0.0f in the lanes beyond nacc
#pragma unroll
        for (int i = 0; i < kNAccMax; ++i) acc[i] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mine, i));
    }
}

// sin(x) for |x| <= pi/2 (odd minimax polynomial, |err| < 1.2e-7 in fp32): the sweep's sin(latitude_field)
// (gclm_pass.hip: row_slat) and the sixth plane of the head epilogue (gclm_fields.hip: pack_fields_kernel), one function
// for both so that a plane written by the epilogue holds the very floats a sweep would compute.  F = float or a 2-wide
// vector of floats (pixel pairs): written with explicit fmas and multiplies only, so v_fma_f32 per float and v_pk_fma_f32
// per pair round alike.  t = x * x.
template <typename F>
__device__ __forceinline__ F sin_halfpi(F x, F t) {
    F p = F(2.6000457182817627e-06f);
    p = __builtin_elementwise_fma(p, t, F(-0.00019806611817330122f));
    p = __builtin_elementwise_fma(p, t, F(0.008333017118275166f));
    p = __builtin_elementwise_fma(p, t, F(-0.16666656732559204f));
    return __builtin_elementwise_fma(x * t, p, x);
}
template <typename F>
__device__ __forceinline__ F sin_halfpi(F x) { return sin_halfpi(x, x * x); }

// The packed confidence plane of a pinhole solve (gclm_pass.hip: row_conf; gclm_api.hip: Plan::cpack): the two confidences of a
// pixel as unsigned 16-bit fixed point in one 32-bit word, the up confidence in the low half.  In numpy, on float32 arrays:
//   q    = np.rint(c * np.float32(65535)).astype(np.uint32)          (float32 product, round half to even)
//   word = q_up | q_lat << 16
//   c'   = q.astype(np.float32) * (np.float32(1) / np.float32(65535))   (the float32 constant, a float32 product)
// conf_encode is defined for c in [0, 1]; anything else (NaN included) is the caller's to keep out (row_conf raises the image's
// flag and never reads the word back).  A confidence that is already c' of some q survives the round trip bit for bit.
constexpr float kConfScale = 65535.0f;
constexpr float kConfStep = 1.0f / 65535.0f;
__device__ __forceinline__ uint32_t conf_encode(float c) { return (uint32_t)rintf(c * kConfScale); }
__device__ __forceinline__ float conf_decode(uint32_t q) { return (float)q * kConfStep; }
__device__ __forceinline__ uint32_t conf_word(uint32_t q_up, uint32_t q_lat) { return q_up | (q_lat << 16); }

#pragma clang fp contract(fast)

}  // namespace dev
}  // namespace gclm
