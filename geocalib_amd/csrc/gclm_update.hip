// gclm_update.hip -- the LM update: per-image / per-group kernels around the sweep (reduction of the workgroup
// partials, lambda rule, damped Cholesky, manifold update, parameter blocks, uncertainty) and the stage kernels
// lm_step / gradient_hessian.  All tiny (O(B) threads); the reference does the same work with a
// device->host->device round trip per step (lm_optimizer.py:128-137).
#include <type_traits>

#include "gclm_device.h"

namespace gclm {

namespace {

using namespace dev;

// The records of the images of a block of kGroups x kSlots threads, summed by the block: unstriped (dev::stripe_of), a
// group is an image and thread (image, slot) walks its records (coalesced over the slots); striped, the block takes ONE
// image and the groups are its stripes.  The per-image leader then owns the sums.
struct CoopRole { Stripe st; int b; bool leader; };      // b: the image of this thread
__host__ __device__ inline int reduce_images_per_block(int nchunks) { return records_striped(nchunks) ? 1 : kGroups; }
inline int reduce_blocks(int B, int nchunks) {
    const int ipb = reduce_images_per_block(nchunks);
    return (B + ipb - 1) / ipb;
}
__device__ inline CoopRole coop_role(int B, int nchunks) {
    const int grp = threadIdx.x / kSlots;
    CoopRole r;
    r.st = stripe_of(nchunks, grp);
    r.b = (int)blockIdx.x * reduce_images_per_block(nchunks) + (r.st.on ? 0 : grp);
    r.leader = r.b < B && threadIdx.x % kSlots == 0 && (!r.st.on || grp == 0);
    return r;
}
// Returns r.leader, whose `acc` holds the sums.  Every thread of the block calls it; launch reduce_blocks(B, nchunks) blocks.
__device__ inline bool coop_reduce_partials(const SolveCtx& c, const CoopRole& r, float (&acc)[kNAccMax]) {
    __shared__ double sacc[kGroups][kSlots + 1];
    const int grp = threadIdx.x / kSlots, slot = threadIdx.x % kSlots, nacc = acc_floats(c.cfg.camera_model);
    const bool active = r.b < c.B && slot < nacc;
    const double sum = sum_records<16>(active, c.partials + (size_t)r.b * c.nchunks * nacc + slot, nacc, r.st.first, r.st.stride, c.nchunks);
    if (active) sacc[grp][slot] = sum;
    __syncthreads();
    if (!r.leader) return false;
#pragma unroll
    for (int i = 0; i < kNAccMax; ++i) {
        double d = 0.0;
        if (i < nacc) {
            if (r.st.on) { for (int g = 0; g < kGroups; ++g) d += sacc[g][i]; }
            else d = sacc[grp][i];
        }
        acc[i] = (float)d;
    }
    return true;
}

// ---------------------------------------------------------------- kernels

__global__ void init_kernel(SolveCtx c, InitArgs ia) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) {
        c.ctrl->stopped = 0;
        c.ctrl->final_sel = c.cfg.num_steps & 1;
        for (int i = 0; i < GCLM_MAX_STEPS + 4; ++i) c.ctrl->notclose[i] = 0;
    }
    if (b >= c.B) return;
    c.cpack_flags[b] = 0;
    const State s = init_state(c, ia, b);
    c.state[0][b] = s;
    PBlock p;
    build_pblock(s, c.cfg.use_spherical_manifold != 0, c.cfg.use_log_focal != 0, p);
    c.pb[0][b] = p;
}

// Independent intrinsics: reduce the partial records, then one thread per image applies the LM step.
// `record` (gclm_solve_recorded): null, or (B, num_steps, GCLM_LM_RECORD_STRIDE) floats; the image's leader leaves row `step`
// there -- the state the step started from, the damping used, the full-size step, "failed", "executed" and the reduced
// accumulator record (include/gclm.h has the layout).  Plain vector stores of values the step computes anyway.
// `sp` (gclm_calibrate_soft): the soft priors' terms join the reduced record before the step (a uniform branch: one
// pointer test per kernel), so the step, the compared cost and the recorded system are the posterior's.
template <int PM>
__global__ __launch_bounds__(kGroups * kSlots) void update_kernel(SolveCtx c, int step, float* record, SoftPrior sp) {
    if (c.cfg.early_stop && stop_fired_before(c.ctrl, step)) return;          // block-uniform
    // the leader of an image fetches its state BEFORE the reduction: the load overlaps the partial records' round trip
    // instead of heading the serial chain behind it
    const CoopRole r = coop_role(c.B, c.nchunks);
    State s{};
    if (r.leader) s = c.state[step & 1][r.b];
    float acc[kNAccMax];
    if (!coop_reduce_partials(c, r, acc)) return;
    const State s0 = s;
    float d[PM];
    bool moved;
    if (sp.on()) {
        const PriorTerms pt = add_soft_priors<PM>(c.cfg, sp, r.b, s, false, false, acc);
        const float pcn = prior_mean(pt.cost, 1.0f / (float)((size_t)c.H * c.W));
        if (step == 0) sp.cost[r.b * 2] = pcn;              // infos["initial_prior_cost"]
        moved = lm_step<PM>(c.cfg, c.H, c.W, step, s, acc, d, &pcn);
        if (pt.bad) s.fails += 1.f;                         // an unusable sigma or prior: its term was left out
    } else {
        moved = lm_step<PM>(c.cfg, c.H, c.W, step, s, acc, d);
    }
    if (moved) atomicAdd(&c.ctrl->notclose[step], 1);
    commit_state(c, step, r.b, s);
    if (record) {
        float* o = record + ((size_t)r.b * c.cfg.num_steps + step) * GCLM_LM_RECORD_STRIDE;
        params_from_state(s0, o + GCLM_LM_RECORD_CAMERA, o + GCLM_LM_RECORD_GRAVITY);
        o[GCLM_LM_RECORD_LAMBDA] = s.lambda;                 // (the rule ran before the solve: the damping this step used)
#pragma unroll
        for (int i = 0; i < GCLM_MAX_PARAMS; ++i) o[GCLM_LM_RECORD_DELTA + i] = i < PM ? d[i < PM ? i : 0] : 0.f;
        o[GCLM_LM_RECORD_FAILED] = s.fails != s0.fails ? 1.f : 0.f;
        o[GCLM_LM_RECORD_EXECUTED] = 1.f;
#pragma unroll
        for (int i = 0; i < kNAccMax; ++i) o[GCLM_LM_RECORD_SYSTEM + i] = acc[i];
    }
}

// Parameter block of the final sweep: (roll, pitch, focal) parametrisation (lm_optimizer.py:481-483).
__global__ void prep_final_kernel(SolveCtx c) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    // which state buffer is final: theta_s if the early stop fired after update s (the tentative theta_{s+1}
    // is discarded, :619-625), else theta_{num_steps}
    const int quiet = c.cfg.early_stop ? first_quiet_step(c.ctrl, c.cfg.num_steps) : c.cfg.num_steps;
    const int sel = quiet & 1, stopped = quiet < c.cfg.num_steps;
    if (b == 0) { c.ctrl->stopped = stopped; c.ctrl->final_sel = sel; }    // for finalize_kernel
    if (b >= c.B) return;
    const State s = c.state[sel][b];
    PBlock p;
    build_pblock(s, false, c.iso_final != 0, p);     // iso_final: log-focal columns, rescaled in finalize_kernel
    c.pb_final[b] = p;
}

// Inverse of an N x N SPD matrix through its Cholesky factor, in double, all sizes compile-time (registers).
// torch.inverse (:484) uses a pivoted LU; on the SPD Hessians of this path both agree to rounding.
template <int N>
__device__ inline void spd_inverse(const float (&A)[N][N], double (&inv)[N][N]) {
    double L[N][N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double sdiag = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) sdiag -= L[j][k] * L[j][k];
        const double l = sqrt(sdiag);
        L[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / l;
        }
    }
#pragma unroll
    for (int col = 0; col < N; ++col) {          // solve L L^T x = e_col
        double x[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double t = i == col ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) t -= L[i][k] * x[k];
            x[i] = t / L[i][i];
        }
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            double t = x[i];
#pragma unroll
            for (int k = i + 1; k < N; ++k) t -= L[k][i] * x[k];
            x[i] = t / L[i][i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) inv[i][col] = x[i];
    }
}

// Final costs + estimate_uncertainty (lm_optimizer.py:632-642, 463-516) from the final sweep.
// `sp`: the soft priors join the final record too -- their cost at the final state the compared cost, their information
// (in the uncertainty sweep's parametrisation) the Hessian before its inverse: the covariance is the posterior's.
template <int PM>
__global__ __launch_bounds__(kGroups * kSlots) void finalize_kernel(SolveCtx c, float* cam, float* grav, float* info, SoftPrior sp) {
    const CoopRole r = coop_role(c.B, c.nchunks);
    const int b = r.b;
    float acc[kNAccMax];
    if (!coop_reduce_partials(c, r, acc)) return;
    const gclm_config& cfg = c.cfg;
    const int sel = c.ctrl->final_sel;
    State s = c.state[sel][b];
    const float invN = 1.0f / (float)((size_t)c.H * c.W);
    float cu, cl;
    float total = total_cost(acc, invN, true, cu, cl);
    float pcn0 = 0.f;
    if (sp.on()) {
        const PriorTerms pt = add_soft_priors<PM>(cfg, sp, b, s, true, c.iso_final != 0, acc);
        const float pcn = prior_mean(pt.cost, invN);
        total = add_prior_mean(total, pcn);
        pcn0 = sp.cost[b * 2];
        sp.cost[b * 2 + 1] = pcn;                           // infos["final_prior_cost"]
    }
    // the final sweep is also the "new cost" evaluation of the last executed step
    const bool update_lambda = !cfg.fix_lambda && !cfg.shared_intrinsics;
    if (!c.ctrl->stopped)
        cost_bookkeeping(cfg, c.ctrl, cfg.num_steps, total, s, update_lambda);
    else if (update_lambda)
        // The stop fired on the comparison of this state's cost with s.prev_cost.  The reference updates lambda BEFORE it
        // tests (:613, :619); that update went into the discarded tentative state, so it is made again here, without the
        // counter: the solve reports the lambda of its fixed-length twin {num_steps: stop_at, early_stop: False}.  (Both
        // launch paths end in this kernel.)
        lambda_rule(total, s);
    float* o = info + (size_t)b * GCLM_INFO_STRIDE;
    for (int i = 0; i < GCLM_INFO_STRIDE; ++i) o[i] = 0.f;      // every slot is written here: no memset by the caller
    o[GCLM_INFO_STOP_AT] = (float)first_quiet_step(c.ctrl, cfg.num_steps);      // (nothing of this launch is needed for it)
    o[GCLM_INFO_INITIAL_UP_COST] = s.init_cu;
    o[GCLM_INFO_INITIAL_LAT_COST] = s.init_cl;
    o[GCLM_INFO_INITIAL_COST] = sp.on() ? add_prior_mean(s.init_cu + s.init_cl, pcn0) : s.init_cu + s.init_cl;
    o[GCLM_INFO_FINAL_UP_COST] = cu;
    o[GCLM_INFO_FINAL_LAT_COST] = cl;
    o[GCLM_INFO_FINAL_COST] = total;
    bool act[PM];
    active_columns<PM>(cfg, act);
    int n = 0;
#pragma unroll
    for (int i = 0; i < PM; ++i) n += act[i] ? 1 : 0;
    o[GCLM_INFO_NPARAMS] = (float)n;
    o[GCLM_INFO_LAMBDA] = s.lambda;
    o[GCLM_INFO_STEP_FAILURES] = s.fails;
    if (cfg.compute_uncertainty) {
        float A[PM][PM], Gf[PM];
        unpack_system<PM>(acc, A, Gf);
        if (c.iso_final) {
            // the final sweep ran the log-focal specialisation (d(u,v)/dlog f = -(u,v)); with fx == fy the plain-focal
            // column of :481-483 is that column times 1/f  (d(u,v)/df = -(u,v)/f)
            const float wf = 1.0f / s.fy;
#pragma unroll
            for (int i = 0; i < PM; ++i) { A[2][i] *= wf; A[i][2] *= wf; }
        }
#pragma unroll
        for (int i = 0; i < PM; ++i)
#pragma unroll
            for (int j = 0; j < PM; ++j)
                if (!(act[i] && act[j])) A[i][j] = i == j ? 1.f : 0.f;
        double Cov[PM][PM];
        spd_inverse<PM>(A, Cov);                              // torch.inverse(Hess), :484
        int ci = 0;                                           // compressed (free-parameter) indices
#pragma unroll
        for (int i = 0; i < PM; ++i) {
            if (!act[i]) continue;
            int cj = 0;
#pragma unroll
            for (int j = 0; j < PM; ++j) {
                if (!act[j]) continue;
                o[GCLM_INFO_COV + ci * n + cj] = (float)Cov[i][j];
                ++cj;
            }
            ++ci;
        }
        if (cfg.estimate_gravity) {
            const double c00 = Cov[0][0], c11 = Cov[1][1], c01 = 0.5 * (Cov[0][1] + Cov[1][0]);
            o[GCLM_INFO_ROLL_UNC] = (float)sqrt(c00);
            o[GCLM_INFO_PITCH_UNC] = (float)sqrt(c11);
            const double tr = 0.5 * (c00 + c11), df = 0.5 * (c00 - c11);
            o[GCLM_INFO_GRAVITY_UNC] = (float)sqrt(tr + sqrt(df * df + c01 * c01));   // max eigvalsh, :495-496
        }
        if (cfg.estimate_focal) {
            const double fu = Cov[2][2];
            const double fy = s.fy, hh = s.h;
            const double Jf = -4.0 * hh / (4.0 * fy * fy + hh * hh);                   // misc.py:285-287
            o[GCLM_INFO_FOCAL_UNC] = (float)(sqrt(fu) * 0.5);
            o[GCLM_INFO_VFOV_UNC] = (float)sqrt(Jf * Jf * fu * 0.5);
        }
    }
    params_from_state(s, cam + (size_t)b * GCLM_CAM_STRIDE, grav + b * 3);
}

// ---------------------------------------------------------------- shared intrinsics
// Whole group = one arrow-head system (lm_optimizer.py:350-383): 2x2 gravity blocks D_i on the
// diagonal, couplings E_i (2 x ni) to the ni shared intrinsics, C = sum H_ii.  Instead of the
// reference's dense (2B+ni)^2 Cholesky the Schur complement on the intrinsics is formed:
//   S = C~ - sum E_i^T D~_i^-1 E_i,  rhs = c - sum E_i^T D~_i^-1 g_i,  delta_I = S^-1 rhs,
//   delta_g,i = D~_i^-1 (g_i - E_i delta_I)         (~ = with LM damping on the diagonal)
// which is algebraically the same solve and reduces over frames with a plain SUM -- i.e. it can
// be all-reduced across devices when a group's frames are sharded (BASELINE config 5).

__device__ inline int lower_bound(const int32_t* a, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ inline void group_range(const SolveCtx& c, int g, int& f0, int& f1) {
    if (c.group_of_frame) { f0 = lower_bound(c.group_of_frame, c.B, g); f1 = lower_bound(c.group_of_frame, c.B, g + 1); }
    else { f0 = g * c.group_size; f1 = min(f0 + c.group_size, c.B); }
}

// Damped 2x2 gravity block of a frame and its inverse; returns false if not positive definite.
template <int PM>
__device__ inline bool frame_block(const float (&Hf)[PM][PM], float lambda, float (&Dinv)[2][2]) {
    const float a = Hf[0][0] + fmaxf(Hf[0][0] * lambda, 1e-6f), b = Hf[0][1], d = Hf[1][1] + fmaxf(Hf[1][1] * lambda, 1e-6f);
    const float det = a * d - b * b;
    if (!(a > 0.f) || !(det > 0.f)) return false;
    const float id = 1.0f / det;
    Dinv[0][0] = d * id; Dinv[0][1] = -b * id; Dinv[1][0] = -b * id; Dinv[1][1] = a * id;
    return true;
}

// Schur partials of one group (ni = 1..3 shared intrinsics), GCLM_SHARED_PARTIAL_STRIDE = 32 floats:
//   [0..9) sum E^T Dinv E (3x3 row-major), [9..12) sum E^T Dinv g, [12..21) sum H_ii, [21..24) sum g_i, [24] #frames;
//   NaN in [0] marks a non-PD frame block.
constexpr int kNI = 3, kGS = 0, kGR = 9, kGC = 12, kGc = 21, kGN = 24, kGSum = 24;

// One frame's step from the REDUCED partials `o` of its group: solve the (tiny) Schur system (redundantly per frame:
// ni <= 3), back-substitute the frame's own gravity block, update (lm_optimizer.py:597-606).
template <int PM, int NI>
__device__ inline void apply_shared_frame(const SolveCtx& c, int step, int b, const float* o) {
    const gclm_config& cfg = c.cfg;
    constexpr int ni = NI;
    State s = c.state[step & 1][b];
    float A[NI][NI], dS[NI], dI[kNI] = {}, dG[2] = {0.f, 0.f};
    bool ok = o[0] == o[0];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        dS[i] = o[kGc + i] - o[kGR + i];
#pragma unroll
        for (int j = 0; j < NI; ++j) A[i][j] = o[kGC + i * kNI + j] - o[kGS + i * kNI + j];
        A[i][i] += fmaxf(o[kGC + i * kNI + i] * s.lambda, 1e-6f);      // damping on sum H_ii (:123-126)
    }
    ok = chol_solve<NI>(A, dS) && ok;
#pragma unroll
    for (int i = 0; i < NI; ++i) dI[i] = dS[i];
    float Hf[PM][PM], Gf[PM], Dinv[2][2];
    unpack_system<PM>(c.frame_sys + (size_t)b * acc_floats(cfg.camera_model), Hf, Gf);
    // Everything that decides about the SHARED step is uniform over the frames of the group (the NaN marker of a
    // non-PD frame block travels in the reduced partials, the Schur solve is the same on every frame): either the
    // whole group takes dI or nobody does -- one camera per group stays one camera per group.
    ok = frame_block<PM>(Hf, s.lambda, Dinv) && ok;
    for (int i = 0; i < ni; ++i) ok = ok && fabsf(dI[i]) <= 3.0e38f;     // NaN / inf: a failed step of the group
    bool frame_failed = false;
    if (ok) {
        float r0 = Gf[0], r1 = Gf[1];
        for (int i = 0; i < ni; ++i) { r0 -= Hf[0][2 + i] * dI[i]; r1 -= Hf[1][2 + i] * dI[i]; }
        dG[0] = Dinv[0][0] * r0 + Dinv[0][1] * r1;
        dG[1] = Dinv[1][0] * r0 + Dinv[1][1] * r1;
        // a frame whose OWN back-substitution overflows keeps its gravity and still follows the group's intrinsics
        frame_failed = !(fabsf(dG[0]) <= 3.0e38f && fabsf(dG[1]) <= 3.0e38f);
        if (frame_failed) dG[0] = dG[1] = 0.f;
    } else {
        for (int i = 0; i < kNI; ++i) dI[i] = 0.f;
    }
    if (!ok || frame_failed) s.fails += 1.f;
    const V3 gv = grav_update({s.gx, s.gy, s.gz}, dG[0], dG[1], cfg.use_spherical_manifold != 0);
    s.gx = gv.x; s.gy = gv.y; s.gz = gv.z;
    update_focal(s, dI[0], cfg.use_log_focal != 0);
    if (ni >= 2) update_dist(s, cfg.camera_model, dI[1], dI[2]);
    commit_state(c, step, b, s);
}

// ONE workgroup per group, cooperative over its frames (tiles of kTileFrames):
//   (1) reduce the sweep's partial records of 8 frames at a time (thread = (frame, slot), fixed chunk order, double),
//   (2) one thread per frame: mean costs / allclose bookkeeping, the frame's damped 2x2 block and its contribution
//       to the group's Schur partials,
//   (3) 24 threads sum the contributions over the frames in frame order (fp32, bit-reproducible),
//   then either write the partials for the all-reduce of the split protocol (APPLY = false: gclm_shared_reduce), or --
//   single device, the partials are already complete -- go straight on to the solve and the per-frame update
//   (APPLY = true): a shared-intrinsics LM step is sweep + THIS kernel, the same two launches as an independent one.
constexpr int kTileFrames = 64;
template <int PM, int NI, bool APPLY>
__global__ __launch_bounds__(kGroups * kSlots) void shared_step_kernel(SolveCtx c, int step, float* gp) {
    if (c.cfg.early_stop && stop_fired_before(c.ctrl, step)) return;          // block-uniform
    const int g = blockIdx.x, tid = threadIdx.x;
    const int nacc = acc_floats(c.cfg.camera_model);
    __shared__ float fsys[kTileFrames][kNAccMax];        // reduced per-frame systems of the tile
    __shared__ float contrib[kTileFrames][kGSum + 1];    // per-frame Schur contributions (+1: bank spread)
    __shared__ int bad[kTileFrames];
    __shared__ float gsum[GCLM_SHARED_PARTIAL_STRIDE];
    int f0, f1;
    group_range(c, g, f0, f1);
    if (tid < GCLM_SHARED_PARTIAL_STRIDE) gsum[tid] = 0.f;
    int any_bad = 0;                                     // thread 0 only
    const int grp = tid / kSlots, slot = tid % kSlots;
    const float invN = 1.0f / (float)((size_t)c.H * c.W);
    for (int t0 = f0; t0 < f1; t0 += kTileFrames) {
        const int nt = min(kTileFrames, f1 - t0);
        // (1) partial records -> fsys (and frame_sys in memory for the apply step)
        for (int base = 0; base < nt; base += kGroups) {
            const int fl = base + grp, b = t0 + fl;
            const bool live = fl < nt && slot < nacc;
            // one ascending walk per frame, never striped: the group's frames are what fills the block here
            const float d = (float)sum_records<16>(live, c.partials + (size_t)b * c.nchunks * nacc + slot, nacc, 0, 1, c.nchunks);
            if (live) {
                fsys[fl][slot] = d;
                c.frame_sys[(size_t)b * nacc + slot] = d;
            }
        }
        __syncthreads();
        // (2) per frame
        if (tid < nt) {
            const int b = t0 + tid;
            State s = c.state[step & 1][b];
            float cu, cl;
            const float total = total_cost(fsys[tid], invN, true, cu, cl);
            if (step == 0) { s.init_cu = cu; s.init_cl = cl; }     // infos["initial_*"] (:585-588)
            cost_bookkeeping(c.cfg, c.ctrl, step, total, s, false);   // lambda is never updated (:612)
            c.state[step & 1][b] = s;
            float Hf[PM][PM], Gf[PM], Dinv[2][2];
            unpack_system<PM>(fsys[tid], Hf, Gf);
            const bool ok = frame_block<PM>(Hf, s.lambda, Dinv);
            bad[tid] = ok ? 0 : 1;
            float* o = contrib[tid];
#pragma unroll
            for (int i = 0; i < kGSum; ++i) o[i] = 0.f;
            const float q0 = Dinv[0][0] * Gf[0] + Dinv[0][1] * Gf[1], q1 = Dinv[1][0] * Gf[0] + Dinv[1][1] * Gf[1];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const float e0 = Hf[0][2 + i], e1 = Hf[1][2 + i];                         // E[:, i]
                const float t0_ = Dinv[0][0] * e0 + Dinv[0][1] * e1, t1_ = Dinv[1][0] * e0 + Dinv[1][1] * e1;
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    o[kGS + j * kNI + i] = Hf[0][2 + j] * t0_ + Hf[1][2 + j] * t1_;
                    o[kGC + i * kNI + j] = Hf[2 + i][2 + j];
                }
                o[kGR + i] = e0 * q0 + e1 * q1;
                o[kGc + i] = Gf[2 + i];
            }
        }
        __syncthreads();
        // (3) sum over the frames of the tile, frame order
        if (tid < kGSum) {
            float a = gsum[tid];
            for (int f = 0; f < nt; ++f) a += contrib[f][tid];
            gsum[tid] = a;
        }
        if (tid == 0)
            for (int f = 0; f < nt; ++f) any_bad |= bad[f];
        __syncthreads();
    }
    if (tid == 0) {
        if (any_bad) gsum[0] = __builtin_nanf("");
        gsum[kGN] = (float)(f1 - f0);
    }
    __syncthreads();
    if constexpr (!APPLY) {
        if (tid < GCLM_SHARED_PARTIAL_STRIDE) gp[(size_t)g * GCLM_SHARED_PARTIAL_STRIDE + tid] = gsum[tid];
    } else {
        for (int b = f0 + tid; b < f1; b += kGroups * kSlots) apply_shared_frame<PM, NI>(c, step, b, gsum);
    }
}

// split protocol, after the all-reduce: per frame, from the REDUCED partials
template <int PM, int NI>
__global__ void shared_apply_kernel(SolveCtx c, int step, const float* gp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.B) return;
    if (c.cfg.early_stop && stop_fired_before(c.ctrl, step)) return;
    const int g = c.group_of_frame ? c.group_of_frame[b] : b / c.group_size;
    apply_shared_frame<PM, NI>(c, step, b, gp + (size_t)g * GCLM_SHARED_PARTIAL_STRIDE);
}

// ---------------------------------------------------------------- gclm_system() helpers

__global__ void pblock_from_params_kernel(SolveCtx c, const float* cam, const float* grav, int as_rpf, PBlock* out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.B) return;
    const State s = state_from_params(cam + (size_t)b * GCLM_CAM_STRIDE, grav + b * 3);
    PBlock p;
    build_pblock(s, c.cfg.use_spherical_manifold && !as_rpf, c.cfg.use_log_focal && !as_rpf, p);
    out[b] = p;
}

template <int PM>
__global__ __launch_bounds__(kGroups * kSlots) void system_out_kernel(SolveCtx c, float* cost, float* grad, float* hess) {
    const CoopRole r = coop_role(c.B, c.nchunks);
    const int b = r.b;
    float acc[kNAccMax];
    if (!coop_reduce_partials(c, r, acc)) return;
    const float invN = 1.0f / (float)((size_t)c.H * c.W);
    cost[b * 2] = acc[A_CU] * invN;
    cost[b * 2 + 1] = acc[A_CL] * invN;
    float Hf[PM][PM], Gf[PM];
    unpack_system<PM>(acc, Hf, Gf);
#pragma unroll
    for (int i = 0; i < GCLM_MAX_PARAMS; ++i) {
        grad[b * GCLM_MAX_PARAMS + i] = i < PM ? Gf[i < PM ? i : 0] : 0.f;
#pragma unroll
        for (int j = 0; j < GCLM_MAX_PARAMS; ++j)
            hess[(b * GCLM_MAX_PARAMS + i) * GCLM_MAX_PARAMS + j] = (i < PM && j < PM) ? Hf[i < PM ? i : 0][j < PM ? j : 0] : 0.f;
    }
}

// optimizer_step (lm_optimizer.py:109-137) as a batched device kernel: delta = (H + diag(clamp(lambda diag H, eps)))^-1 G
// by an fp32 Cholesky per system (the reference copies H, G to the CPU for this, twice per LM step).  A system
// that is not positive definite takes a zero step and raises its flag (the reference zeroes the whole batch).
template <int N>
__global__ void lm_step_kernel(const float* G, const float* H, const float* lambda, int lambda_stride, float eps, int B,
                               float* delta, int* failed) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float A[N][N], g[N];
    const float lam = lambda[(size_t)b * lambda_stride];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        g[i] = G[(size_t)b * N + i];
#pragma unroll
        for (int j = 0; j < N; ++j) A[i][j] = H[((size_t)b * N + i) * N + j];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) A[i][i] += fmaxf(A[i][i] * lam, eps);
    const bool ok = chol_solve<N>(A, g);
#pragma unroll
    for (int i = 0; i < N; ++i) delta[(size_t)b * N + i] = ok ? g[i] : 0.f;
    if (failed) failed[b] = ok ? 0 : 1;
}

// calculate_gradient_and_hessian (lm_optimizer.py:317-385) on MATERIALISED tensors: G = sum_px w J^T r,
// H = sum_px w J^T J for J (B,N,R,P), r (B,N,R), w (B,N).  One workgroup per image, fixed summation order
// (per-thread strided partial sums in double, then a tree over the 256 threads in LDS).  The solve itself never
// forms J; this serves callers that hold the tensors.
template <int P>
__global__ __launch_bounds__(256) void gradient_hessian_kernel(const float* J, const float* r, const float* w, int N,
                                                               int R, int accumulate, float* G, float* H) {
    constexpr int NV = P + P * (P + 1) / 2;
    const int b = blockIdx.x, tid = threadIdx.x;
    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;
    for (int px = tid; px < N; px += 256) {
        const size_t q = (size_t)b * N + px;
        const float wt = w[q];
        for (int row = 0; row < R; ++row) {
            const float* j = J + (q * R + row) * P;
            const float res = r[q * R + row];
            float jr[P];
#pragma unroll
            for (int k = 0; k < P; ++k) jr[k] = j[k];
            int o = P;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const float wk = wt * jr[k];
                acc[k] += (double)(wk * res);
#pragma unroll
                for (int l = k; l < P; ++l) acc[o++] += (double)(wk * jr[l]);
            }
        }
    }
    __shared__ double red[256];
    double total[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        red[tid] = acc[i];
        __syncthreads();
        for (int sft = 128; sft > 0; sft >>= 1) {
            if (tid < sft) red[tid] += red[tid + sft];
            __syncthreads();
        }
        total[i] = red[0];
        __syncthreads();
    }
    if (tid != 0) return;
    int o = P;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        float* g = G + (size_t)b * P + k;
        *g = (accumulate ? *g : 0.f) + (float)total[k];
#pragma unroll
        for (int l = k; l < P; ++l) {
            const float v = (float)total[o++];
            float* hkl = H + ((size_t)b * P + k) * P + l;
            float* hlk = H + ((size_t)b * P + l) * P + k;
            const float nv = (accumulate ? *hkl : 0.f) + v;
            *hkl = nv;
            *hlk = nv;
        }
    }
}

inline dim3 grid1(int n) { return dim3((n + 127) / 128); }

}  // namespace

#define GCLM_L(kernel, n, s, ...) hipLaunchKernelGGL(kernel, grid1(n), dim3(128), 0, s, __VA_ARGS__)
// cooperative-reduce kernels: 256-thread blocks of 8 images (or 1 striped image, see coop_role)
#define GCLM_LR(kernel, n, s, ...) \
    hipLaunchKernelGGL(kernel, dim3(reduce_blocks((n), c.nchunks)), dim3(kGroups * kSlots), 0, s, __VA_ARGS__)
// one block per group of shared intrinsics
#define GCLM_LG(kernel, s, ...) hipLaunchKernelGGL(kernel, dim3(c.n_groups), dim3(kGroups * kSlots), 0, s, __VA_ARGS__)

// The one place a camera model becomes the sizes these kernels are instantiated for: f(pm, ni) gets PM, the full columns of
// a record's system (acc_pm), and NI, the intrinsics a group shares (focal + distortion), as integral constants; whatever
// f launches, its launch error is returned.
template <typename F>
hipError_t with_system_size(int camera_model, F&& f) {
    return with_camera_model(camera_model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        f(std::integral_constant<int, acc_pm(M)>{}, std::integral_constant<int, 1 + num_dist_params(M)>{});
        return hipGetLastError();
    });
}

hipError_t launch_init(const SolveCtx& c, const InitArgs& ia, hipStream_t s) {
    GCLM_L(init_kernel, c.B > 0 ? c.B : 1, s, c, ia);     // B = 0 (an empty shard of the split protocol): thread 0 still resets Ctrl
    return hipGetLastError();
}
hipError_t launch_update(const SolveCtx& c, int step, hipStream_t s, float* d_record, const SoftPrior& sp) {
    return with_system_size(c.cfg.camera_model, [&](auto pm, auto) { GCLM_LR(update_kernel<pm>, c.B, s, c, step, d_record, sp); });
}
hipError_t launch_prep_final(const SolveCtx& c, hipStream_t s) {
    GCLM_L(prep_final_kernel, c.B, s, c);
    return hipGetLastError();
}
hipError_t launch_finalize(const SolveCtx& c, float* d_cam, float* d_grav, float* d_info, hipStream_t s, const SoftPrior& sp) {
    return with_system_size(c.cfg.camera_model, [&](auto pm, auto) { GCLM_LR(finalize_kernel<pm>, c.B, s, c, d_cam, d_grav, d_info, sp); });
}
// Parts of ONE batch solved by separate handles (LMOptimizer.overlap_streams): infos["stop_at"] is a property of the
// whole batch, so it is re-derived from the SUM of the parts' per-step counters and written into every row of every part.
__global__ void merge_stop_kernel(MergeStopArgs a) {
    __shared__ int stop;
    if (threadIdx.x == 0) stop = dev::first_quiet_step(a.ctrl, a.n, a.num_steps);
    __syncthreads();
    const float v = (float)stop;
    for (int p = 0; p < a.n; ++p)
        for (int i = threadIdx.x; i < a.B[p]; i += blockDim.x) a.info[p][(size_t)i * GCLM_INFO_STRIDE + GCLM_INFO_STOP_AT] = v;
}
hipError_t launch_merge_stop(const MergeStopArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(merge_stop_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_shared_reduce(const SolveCtx& c, int step, float* d_group_partials, hipStream_t s) {
    if (c.n_groups <= 0) return hipSuccess;
    return with_system_size(c.cfg.camera_model, [&](auto pm, auto ni) { GCLM_LG((shared_step_kernel<pm, ni, false>), s, c, step, d_group_partials); });
}
// single device: reduce + solve + update of every group in ONE launch
hipError_t launch_shared_step(const SolveCtx& c, int step, hipStream_t s) {
    if (c.n_groups <= 0) return hipSuccess;
    return with_system_size(c.cfg.camera_model, [&](auto pm, auto ni) { GCLM_LG((shared_step_kernel<pm, ni, true>), s, c, step, nullptr); });
}
hipError_t launch_shared_apply(const SolveCtx& c, int step, const float* d_group_partials, hipStream_t s) {
    return with_system_size(c.cfg.camera_model, [&](auto pm, auto ni) { GCLM_L((shared_apply_kernel<pm, ni>), c.B, s, c, step, d_group_partials); });
}
hipError_t launch_system_out(const SolveCtx& c, float* d_cost, float* d_grad, float* d_hess, hipStream_t s) {
    return with_system_size(c.cfg.camera_model, [&](auto pm, auto) { GCLM_LR(system_out_kernel<pm>, c.B, s, c, d_cost, d_grad, d_hess); });
}
hipError_t launch_pblock_from_params(const SolveCtx& c, const float* d_cam, const float* d_grav, int as_rpf,
                                     PBlock* out, hipStream_t s) {
    GCLM_L(pblock_from_params_kernel, c.B, s, c, d_cam, d_grav, as_rpf, out);
    return hipGetLastError();
}

hipError_t launch_lm_step(const float* d_G, const float* d_H, const float* d_lambda, int lambda_stride, float eps, int B,
                          int P, float* d_delta, int* d_failed, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    switch (P) {
#define GCLM_STEP(N) \
    case N: hipLaunchKernelGGL(lm_step_kernel<N>, grid1(B), dim3(128), 0, s, d_G, d_H, d_lambda, lambda_stride, eps, B, d_delta, d_failed); break
        GCLM_STEP(1); GCLM_STEP(2); GCLM_STEP(3); GCLM_STEP(4); GCLM_STEP(5);
#undef GCLM_STEP
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_gradient_hessian(const float* d_J, const float* d_r, const float* d_w, int B, int N, int R, int P,
                                   int accumulate, float* d_G, float* d_H, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    switch (P) {
#define GCLM_GH(K) \
    case K: hipLaunchKernelGGL(gradient_hessian_kernel<K>, dim3(B), dim3(256), 0, s, d_J, d_r, d_w, N, R, accumulate, d_G, d_H); break
        GCLM_GH(1); GCLM_GH(2); GCLM_GH(3); GCLM_GH(4); GCLM_GH(5);
#undef GCLM_GH
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gclm
