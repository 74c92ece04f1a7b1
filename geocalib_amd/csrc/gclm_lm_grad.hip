// gclm_lm_grad.hip -- gclm_lm_backward: the adjoint of the LM steps of a recorded solve (gclm_solve_recorded), i.e. the
// gradients of the optimised camera and gravity with respect to the up field, the latitude field and the two confidence maps
// (the reference's training-time optimiser gets them from autograd through every step, with (B, N, 3, P) Jacobians kept alive
// per step; siclib/models/optimization/lm_optimizer.py).  include/gclm.h: gclm_lm_backward has the mathematics.
//
// Per step, last executed first, three launches:
//   lm_grad_prepare_kernel   one thread per image, in float64 (O(B) work; the pixel pass inherits every rounding made here).
//                            The adjoint of theta [+] delta in forward mode (Dual<double, 9>: five state components, four
//                            step components), v = A^-1 delta-bar by a Cholesky on the recorded system damped as the forward
//                            damped it, the clamp mask; and the jets of the parameters the pixel code reads -- gravity,
//                            1 / fx, 1 / fy, k1 at theta [+] delta', delta' = 0 -- as Dual<Dual<double, 1>, P>, stored as
//                            floats: the inner level over the P columns of delta' (the Jacobian), the outer over ONE state
//                            component, one set per component.
//   lm_grad_pixel_kernel     the tile walk of gclm_render.h at one pixel per lane (ragged tiles masked), in float64.  A lane
//                            evaluates the up field and sin(latitude) of its pixel in jet arithmetic from the parameter jets:
//                            value, Jacobian columns and their derivative with respect to the state component of the pass, for
//                            each component in turn (the jets are block-uniform loads), so that a pass holds 2 (1 + P) floats
//                            per quantity, not (1 + 5)(1 + P).  phi's derivative with respect to the component is summed per
//                            lane, wave (wave_sum's butterfly, written out on doubles), block (tile_record) into one record per tile; the first pass also forms the
//                            derivatives with respect to the pixel's own inputs and stores them, or adds them to the plane
//                            (the first processed step stores: no memset).  No atomics.
//   lm_grad_finish_kernel    one block per image: the tile records summed in float64 in a fixed order, plus the direct term.
// A step at or after the early stop returns at once in all three (block-uniform).  A gradient plane that is NULL is neither
// computed nor written.  Pinhole and simple_radial, spherical manifold, log focal length.
#include "gclm_device.h"
#include "gclm_render.h"

namespace gclm {
namespace {

using namespace dev;

// ---------------------------------------------------------------- forward-mode numbers
// v + sum_i d[i] eps_i, eps_i eps_j = 0; T = float, or a Dual again (second derivatives, mixed only).
template <typename T, int N>
struct Dual {
    T v;
    T d[N];
    __device__ __forceinline__ Dual() {}
    __device__ __forceinline__ Dual(float x) : v(x) {
#pragma unroll
        for (int i = 0; i < N; ++i) d[i] = T(0.f);
    }
};

__device__ __forceinline__ float value(float x) { return x; }
__device__ __forceinline__ float value(double x) { return (float)x; }
template <typename T, int N>
__device__ __forceinline__ float value(const Dual<T, N>& a) { return value(a.v); }

#define GCLM_DUAL template <typename T, int N> __device__ __forceinline__ Dual<T, N>
GCLM_DUAL operator+(const Dual<T, N>& a, const Dual<T, N>& b) {
    Dual<T, N> o;
    o.v = a.v + b.v;
#pragma unroll
    for (int i = 0; i < N; ++i) o.d[i] = a.d[i] + b.d[i];
    return o;
}
GCLM_DUAL operator-(const Dual<T, N>& a, const Dual<T, N>& b) {
    Dual<T, N> o;
    o.v = a.v - b.v;
#pragma unroll
    for (int i = 0; i < N; ++i) o.d[i] = a.d[i] - b.d[i];
    return o;
}
GCLM_DUAL operator-(const Dual<T, N>& a) {
    Dual<T, N> o;
    o.v = -a.v;
#pragma unroll
    for (int i = 0; i < N; ++i) o.d[i] = -a.d[i];
    return o;
}
GCLM_DUAL operator*(const Dual<T, N>& a, const Dual<T, N>& b) {
    Dual<T, N> o;
    o.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < N; ++i) o.d[i] = a.d[i] * b.v + a.v * b.d[i];
    return o;
}
GCLM_DUAL operator*(const Dual<T, N>& a, float b) {
    Dual<T, N> o;
    o.v = a.v * b;
#pragma unroll
    for (int i = 0; i < N; ++i) o.d[i] = a.d[i] * b;
    return o;
}
GCLM_DUAL operator*(float b, const Dual<T, N>& a) { return a * b; }
GCLM_DUAL operator+(const Dual<T, N>& a, float b) {
    Dual<T, N> o = a;
    o.v = a.v + b;
    return o;
}
GCLM_DUAL operator+(float b, const Dual<T, N>& a) { return a + b; }
GCLM_DUAL operator-(const Dual<T, N>& a, float b) { return a + (-b); }
GCLM_DUAL operator-(float b, const Dual<T, N>& a) { return (-a) + b; }

__device__ __forceinline__ float rcp_(float x) { return 1.f / x; }
__device__ __forceinline__ float sqrt_(float x) { return sqrtf(x); }
__device__ __forceinline__ float exp_(float x) { return expf(x); }
__device__ __forceinline__ float sin_(float x) { return sinf(x); }
__device__ __forceinline__ float cos_(float x) { return cosf(x); }
__device__ __forceinline__ double rcp_(double x) { return 1.0 / x; }
__device__ __forceinline__ double sqrt_(double x) { return sqrt(x); }
__device__ __forceinline__ double exp_(double x) { return exp(x); }
__device__ __forceinline__ double sin_(double x) { return sin(x); }
__device__ __forceinline__ double cos_(double x) { return cos(x); }
// f(a) with f'(a) = m: the chain rule once
GCLM_DUAL chain(const Dual<T, N>& a, const T& fv, const T& m) {
    Dual<T, N> o;
    o.v = fv;
#pragma unroll
    for (int i = 0; i < N; ++i) o.d[i] = a.d[i] * m;
    return o;
}
GCLM_DUAL rcp_(const Dual<T, N>& a) {
    const T r = rcp_(a.v);
    return chain(a, r, -(r * r));
}
GCLM_DUAL sqrt_(const Dual<T, N>& a) {          // (the slope at 0 is taken as 0, as torch takes the norm's)
    const T s = sqrt_(a.v);
    return chain(a, s, value(s) > 0.f ? rcp_(s) * 0.5f : T(0.f));
}
GCLM_DUAL exp_(const Dual<T, N>& a) {
    const T e = exp_(a.v);
    return chain(a, e, e);
}
GCLM_DUAL sin_(const Dual<T, N>& a) { return chain(a, sin_(a.v), cos_(a.v)); }
GCLM_DUAL cos_(const Dual<T, N>& a) { return chain(a, cos_(a.v), -sin_(a.v)); }
#undef GCLM_DUAL

// ---------------------------------------------------------------- theta [+] delta, on any number type
// SphericalManifold.householder_vector / plus (misc.py:182-259; gclm_device.h: householder, grav_update_post) and the
// normalisation of Gravity's constructor; `e` is exp(delta): (sinc d0, sinc d1, cos |d|), or (d0, d1, 1) to first order at 0.
template <typename T>
__device__ __forceinline__ void gravity_plus(const T (&g)[3], const T (&e)[3], T (&out)[3]) {
    T sigma = g[0] * g[0] + g[1] * g[1];
    const T norm = sqrt_(sigma + g[2] * g[2]);
    if (value(sigma) < 1e-7f) sigma = sigma + 1e-7f;
    const T vpiv = value(g[2]) < 0.f ? g[2] - norm : -(sigma * rcp_(g[2] + norm));
    const T beta = (vpiv * vpiv) * 2.f * rcp_(sigma + vpiv * vpiv);
    const T iv = rcp_(vpiv);
    const T v[3] = {g[0] * iv, g[1] * iv, T(1.f)};
    const T bd = beta * (v[0] * e[0] + v[1] * e[1] + v[2] * e[2]);
    T y[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = norm * (e[i] - v[i] * bd);
    const T in = rcp_(sqrt_(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]));
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = y[i] * in;
}

// ---------------------------------------------------------------- the fields of one pixel, on any number type
// (gclm_render.h: persp_up normalised, persp_lat before its asin -- the formulas of perspective_fields.py:47-81, 185-211)
template <typename T>
struct Params {
    T a, b, c, ifx, ify, k1;
};
constexpr int kParamJets = 6;

template <int MODEL, typename T>
__device__ __forceinline__ void pixel_fields(const Params<T>& p, float xc, float yc, bool want_up, T& upx, T& upy, T& sl) {
    const T u = p.ifx * xc, v = p.ify * yc;
    const T r2 = u * u + v * v;
    if (want_up) {
        const T px = p.a - p.c * u, py = p.b - p.c * v;
        T qx = px, qy = py;
        if constexpr (MODEL != GCLM_PINHOLE) {       // simple_radial: s = 1 + k1 r2, s' = k1
            const T s = p.k1 * r2 + 1.f;
            const T o = p.k1 * (u * px + v * py) * 2.f;
            qx = s * px + o * u;
            qy = s * py + o * v;
        }
        const T in = rcp_(sqrt_(qx * qx + qy * qy));
        upx = qx * in;
        upy = qy * in;
    }
    T X = u, Y = v;
    if constexpr (MODEL != GCLM_PINHOLE) {
        const T t = 1.f - p.k1 * r2;
        X = u * t;
        Y = v * t;
    }
    sl = (X * p.a + Y * p.b + p.c) * rcp_(sqrt_(X * X + Y * Y + 1.f));
    if (value(sl) < -kLatHi) sl = T(-kLatHi);        // the clamp of get_latitude_field: a constant beyond it
    if (value(sl) > kLatHi) sl = T(kLatHi);
}

// ---------------------------------------------------------------- layout of a call
constexpr int kAdj = 5;                 // state adjoint: gravity (3), fy (fx follows at a fixed ratio), k1
constexpr int kAdjStride = 8;
constexpr int kStepWords = 16;          // per image and step: v[4], delta[4], lambda m[4], cx, cy, pad
template <int MODEL> constexpr int inner_cols() { return MODEL == GCLM_PINHOLE ? 3 : 4; }
template <int MODEL> constexpr int state_words() { return MODEL == GCLM_PINHOLE ? 4 : 5; }
constexpr int kJetFloatsMax = 2 * (1 + 4);
constexpr int kParamFloats = kAdj * kParamJets * kJetFloatsMax;        // per image: one set of parameter jets per state component

struct GradCall {
    const float *up, *lat, *upc, *latc, *record, *info, *grad_cam, *grad_grav;
    float *g_up, *g_lat, *g_upc, *g_latc;
    float *adj, *direct, *stepc, *params;              // workspace
    double* rec;                                       // ... its tile records
    int B, H, W, tiles_x, tiles, num_steps, early_stop;
    int eg, ef, ed;
    float up_scale, lat_scale;
};

// Steps [0, last_step) are the solve.  The early stop is ONE decision over the whole call (the reference's allclose over the
// batch; gclm_update.hip writes the same stop_at into every image's info row), so image 0's row speaks for all of them.
__device__ __forceinline__ int last_step(const GradCall& a) {
    return a.early_stop ? min((int)a.info[GCLM_INFO_STOP_AT], a.num_steps) : a.num_steps;
}

// ---------------------------------------------------------------- per image
template <int MODEL>
__global__ __launch_bounds__(64) void lm_grad_prepare_kernel(const GradCall a, int step) {
    const int last = last_step(a);
    if (step >= last) return;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    constexpr int P = inner_cols<MODEL>(), NK = state_words<MODEL>();
    const float* rc = a.record + ((size_t)b * a.num_steps + step) * GCLM_LM_RECORD_STRIDE;
    const float* cm = rc + GCLM_LM_RECORD_CAMERA;
    const float g0[3] = {rc[GCLM_LM_RECORD_GRAVITY], rc[GCLM_LM_RECORD_GRAVITY + 1], rc[GCLM_LM_RECORD_GRAVITY + 2]};
    const float fx = cm[2], fy = cm[3], k1 = cm[6], ratio = fx / fy, hgt = cm[1];
    const float lambda = rc[GCLM_LM_RECORD_LAMBDA];
    const bool failed = rc[GCLM_LM_RECORD_FAILED] != 0.f;
    float d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = rc[GCLM_LM_RECORD_DELTA + i];
    const bool has_dist = MODEL != GCLM_PINHOLE;
    const bool act[4] = {a.eg != 0, a.eg != 0, a.ef != 0, has_dist};
    // the steps update_estimate applies (gclm_device.h: split_delta, with its quirk: without a free focal length the
    // distortion takes the first gravity step)
    const bool dist_own = a.ef || !a.eg;
    const float dg0 = a.eg ? d[0] : 0.f, dg1 = a.eg ? d[1] : 0.f, df = a.ef ? d[2] : 0.f, dk = dist_own ? d[3] : d[0];
    const bool dist_moves = has_dist && a.ed;

    // incoming adjoint: of the outputs at the first processed step, else what the finish kernel left
    float in[kAdj];
    if (step == last - 1) {
        const float* gc = a.grad_cam + (size_t)b * 8;
        in[0] = a.grad_grav[b * 3], in[1] = a.grad_grav[b * 3 + 1], in[2] = a.grad_grav[b * 3 + 2];
        in[3] = gc[3] + gc[2] * ratio;
        in[4] = has_dist ? gc[6] + gc[7] : 0.f;         // (slot 7 shadows k1 for one-parameter models)
    } else {
#pragma unroll
        for (int k = 0; k < kAdj; ++k) in[k] = a.adj[(size_t)b * kAdjStride + k];
    }

    // (1) the adjoint of theta+ = theta [+] delta: tangents 0..4 the state, 5..8 the applied steps
    using D9 = Dual<double, 9>;
    auto seed = [](float v, int i) { D9 t(v); t.d[i] = 1.0; return t; };
    const D9 g[3] = {seed(g0[0], 0), seed(g0[1], 1), seed(g0[2], 2)};
    const D9 s0 = seed(dg0, 5), s1 = seed(dg1, 6);
    const D9 nd2 = s0 * s0 + s1 * s1, nd = sqrt_(nd2);
    D9 e[3];
    if (value(nd) < 1e-7f) {
        e[0] = s0, e[1] = s1, e[2] = cos_(nd);
    } else {
        const D9 sinc = sin_(nd) * rcp_(nd);
        e[0] = sinc * s0, e[1] = sinc * s1, e[2] = cos_(nd);
    }
    D9 out[kAdj];
    {
        D9 gp[3];
        gravity_plus<D9>(g, e, gp);
        out[0] = gp[0], out[1] = gp[1], out[2] = gp[2];
    }
    {
        D9 f = seed(fy, 3) * exp_(seed(df, 7));           // exp(log fy + delta_f)
        const float lo = hgt * 0.5f / 3.7320504f, hi = hgt * 0.5f / 0.043660942f;
        if (value(f) < lo) f = D9(lo);
        if (value(f) > hi) f = D9(hi);
        out[3] = f;
        D9 k = seed(k1, 4);
        if (dist_moves) {
            k = k + seed(dk, 8);
            if (value(k) < -0.7f) k = D9(-0.7f);
            if (value(k) > 0.7f) k = D9(0.7f);
        }
        out[4] = k;
    }
    double direct[kAdj], sbar[4];
#pragma unroll
    for (int k = 0; k < kAdj; ++k) {
        double t = 0.0;
#pragma unroll
        for (int o = 0; o < kAdj; ++o) t += in[o] * out[o].d[k];
        direct[k] = t;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double t = 0.0;
#pragma unroll
        for (int o = 0; o < kAdj; ++o) t += in[o] * out[o].d[5 + j];
        sbar[j] = t;
    }
    // ... into the columns of the solve (the adjoint of split_delta)
    double v[4] = {a.eg ? sbar[0] : 0.0, a.eg ? sbar[1] : 0.0, a.ef ? sbar[2] : 0.0, 0.0};
    if (dist_moves) {
        if (dist_own) v[3] = sbar[3]; else v[0] += sbar[3];
    }
    // (2) v = A^-1 delta-bar on the recorded system, damped as the forward damped it (gclm_device.h: lm_solve)
    float Af[4][4], Gd[4], lm[4];
    double A[4][4];
    unpack_system<4>(rc + GCLM_LM_RECORD_SYSTEM, Af, Gd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        lm[i] = (act[i] && Af[i][i] * lambda > 1e-6f) ? lambda : 0.f;      // the forward's float32 test
#pragma unroll
        for (int j = 0; j < 4; ++j) A[i][j] = (act[i] && act[j]) ? (double)Af[i][j] : (i == j ? 1.0 : 0.0);
        if (act[i]) A[i][i] += (double)fmaxf(Af[i][i] * lambda, 1e-6f); else v[i] = 0.0;
    }
    bool ok = !failed;
#pragma unroll
    // (not dev::chol_solve on doubles: gclm_device.h switches contraction off, this file has it on -- other float64 roundings)
    for (int j = 0; j < 4; ++j) {                // in-place Cholesky solve (gclm_device.h: chol_solve), in float64
        double t = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) t -= A[j][k] * A[j][k];
        ok = ok && t > 0.0;
        const double l = sqrt(t);
        A[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double u = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) u -= A[i][k] * A[j][k];
            A[i][j] = u / l;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double t = v[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= A[i][k] * v[k];
        v[i] = t / A[i][i];
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        double t = v[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) t -= A[k][i] * v[k];
        v[i] = t / A[i][i];
    }
    float* sc = a.stepc + (size_t)b * kStepWords;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sc[i] = ok ? (float)v[i] : 0.f;
        sc[4 + i] = act[i] ? d[i] : 0.f;
        sc[8 + i] = lm[i];
    }
    sc[12] = cm[4], sc[13] = cm[5];
#pragma unroll
    for (int k = 0; k < kAdj; ++k) a.direct[(size_t)b * kAdjStride + k] = (float)direct[k];

    // (3) the parameter jets at theta [+] delta', delta' = 0, one set per state component
    using D1 = Dual<double, 1>;
    using J = Dual<D1, P>;
    for (int k = 0; k < NK; ++k) {
        auto st = [&](float val, int i) { D1 t(val); t.d[0] = i == k ? 1.0 : 0.0; J o; o.v = t;
#pragma unroll
            for (int j = 0; j < P; ++j) o.d[j] = D1(0.f);
            return o; };
        auto col = [&](int j) { J o(0.f); o.d[j] = D1(1.f); return o; };
        const J gg[3] = {st(g0[0], 0), st(g0[1], 1), st(g0[2], 2)};
        const J ee[3] = {col(0), col(1), J(1.f)};
        J gp[3];
        gravity_plus<J>(gg, ee, gp);
        const J f = st(fy, 3) * exp_(col(2));
        Params<J> p;
        p.a = gp[0], p.b = gp[1], p.c = gp[2];
        p.ify = rcp_(f);
        p.ifx = p.ify * (float)(1.0 / (double)ratio);
        p.k1 = st(k1, 4);
        if constexpr (P > 3) p.k1 = p.k1 + col(3);
        float* o = a.params + ((size_t)b * kAdj + k) * kParamJets * kJetFloatsMax;
        const J* jets[kParamJets] = {&p.a, &p.b, &p.c, &p.ifx, &p.ify, &p.k1};
#pragma unroll
        for (int q = 0; q < kParamJets; ++q) {
            float* w = o + q * kJetFloatsMax;
            w[0] = (float)jets[q]->v.v, w[1] = (float)jets[q]->v.d[0];
#pragma unroll
            for (int j = 0; j < P; ++j) w[2 + 2 * j] = (float)jets[q]->d[j].v, w[3 + 2 * j] = (float)jets[q]->d[j].d[0];
        }
    }
}

// ---------------------------------------------------------------- per pixel
// The weight of a field's residual r (C components) under the reference's scaled Huber loss (lm_optimizer.py:61-87):
// w = conf rho'(x), x = |r|^2 / a^2, rho' = 1 (x <= 1), else max(eps, 1 / sqrt(x + 1e-8)).  Handed out as
//   w      the weight, a number of the pass;
//   psi_c  = w r_c, with its derivative in CLOSED form: in the outer branch d(w r_c) = conf rho' (dr_c - r_c (r . dr) /
//          (|r|^2 + 1e-8 a^2)) -- the product rule's two terms, w dr_c and r_c dw, cancel along r (all of them for the
//          one-component latitude residual, where what is left is conf 1e-8 rho'^3 dr), which float32 pays for with the
//          digits of every outlier;
//   rho1 = rho', drho = conf rho'' 2 / a^2 (dw/dr_c = drho r_c), and proj = the denominator above (0: no projection).
using D1 = Dual<float, 1>;
constexpr float kF32Eps = 1.1920928955078125e-07f;
template <int C>
struct Weighted {
    D1 w, psi[C];
    float rho1, drho, proj;
};
template <int C>
__device__ __forceinline__ Weighted<C> huber_weighted(const D1 (&r)[C], float inv_a2, float conf) {
    Weighted<C> o;
    float sq = 0.f, dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) sq += r[c].v * r[c].v, dot += r[c].v * r[c].d[0];
    const float x = sq * inv_a2;
    const float isx = 1.f / sqrtf(x + 1e-8f);
    const bool inlier = x <= 1.f, floor_ = !inlier && isx < kF32Eps;
    o.rho1 = inlier ? 1.f : (floor_ ? kF32Eps : isx);
    const float rho2 = (inlier || floor_) ? 0.f : -0.5f * isx * isx * isx;
    o.drho = conf * rho2 * 2.f * inv_a2;
    o.proj = (inlier || floor_) ? 0.f : sq + 1e-8f / inv_a2;
    o.w.v = conf * o.rho1;
    o.w.d[0] = o.drho * dot;
    const float cw = conf * o.rho1;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        o.psi[c].v = cw * r[c].v;
        if (o.proj == 0.f) o.psi[c].d[0] = cw * r[c].d[0];
        else if (C == 1) o.psi[c].d[0] = conf * 1e-8f * isx * isx * isx * r[c].d[0];
        else o.psi[c].d[0] = cw * (r[c].d[0] - r[c].v * (dot / o.proj));
    }
    return o;
}
// d(sum_c jv_c psi_c)/dr_c at fixed jv: the same closed form along the direction jv
template <int C>
__device__ __forceinline__ float psi_grad(const Weighted<C>& h, const D1 (&r)[C], const float (&jv)[C], float conf, int c) {
    const float cw = conf * h.rho1;
    if (h.proj == 0.f) return cw * jv[c];
    if (C == 1) return conf * 1e-8f * h.rho1 * h.rho1 * h.rho1 * jv[c];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < C; ++i) dot += r[i].v * jv[i];
    return cw * (jv[c] - r[c].v * (dot / h.proj));
}

template <int MODEL>
__global__ __launch_bounds__(kBlock) void lm_grad_pixel_kernel(const GradCall a, int step) {
    constexpr int P = inner_cols<MODEL>(), NK = state_words<MODEL>();
    using J = Dual<D1, P>;
    __shared__ double s_sum[kTileRows][kAdj];
    const int last = last_step(a);
    if (step >= last) return;                              // block-uniform
    const bool store = step == last - 1;                   // the first processed step stores, later ones accumulate
    const int nk = step == 0 ? 1 : NK;                     // the initial estimate takes no gradient: its adjoint is not formed
    int x, y;
    const bool in = tile_pixel<1>(a.tiles_x, a.H, a.W, x, y);
    const int b = blockIdx.y, wave = threadIdx.x >> 6;
    const float* sc = a.stepc + (size_t)b * kStepWords;
    float v[P], dl[P], lmvd[P];
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = sc[j], dl[j] = sc[4 + j], lmvd[j] = sc[8 + j] * sc[j] * sc[4 + j];
    const float xc = (float)x - sc[12], yc = (float)y - sc[13];
    const size_t hw = (size_t)a.H * a.W, o = in ? (size_t)b * hw + (size_t)y * a.W + x : 0;
    float dux = 0.f, duy = 0.f, dlat = 0.f, cu = 1.f, cl = 1.f;
    if (in) {
        if (a.up) dux = a.up[o + (size_t)b * hw], duy = a.up[o + (size_t)b * hw + hw];
        dlat = a.lat[o];
        if (a.up && a.upc) cu = a.upc[o];
        if (a.latc) cl = a.latc[o];
    }
    const float slat = sinf(dlat);
    const float iau = 1.f / (a.up_scale * a.up_scale), ial = 1.f / (a.lat_scale * a.lat_scale);
    double sum[kAdj] = {0.0, 0.0, 0.0, 0.0, 0.0};       // (the terms of a state component cancel across pixels: summed in float64)
#pragma unroll 1
    for (int k = 0; k < nk; ++k) {
        Params<J> p;
        {
            const float* pj = a.params + ((size_t)b * kAdj + k) * kParamJets * kJetFloatsMax;
            J* jets[kParamJets] = {&p.a, &p.b, &p.c, &p.ifx, &p.ify, &p.k1};
#pragma unroll
            for (int q = 0; q < kParamJets; ++q) {
                const float* w = pj + q * kJetFloatsMax;
                jets[q]->v.v = w[0], jets[q]->v.d[0] = w[1];
#pragma unroll
                for (int j = 0; j < P; ++j) jets[q]->d[j].v = w[2 + 2 * j], jets[q]->d[j].d[0] = w[3 + 2 * j];
            }
        }
        J upx(0.f), upy(0.f), sl;
        pixel_fields<MODEL, J>(p, xc, yc, a.up != nullptr, upx, upy, sl);
        D1 phi(0.f);
        if (a.up) {
            const D1 r[2] = {dux - upx.v, duy - upy.v};
            const Weighted<2> h = huber_weighted<2>(r, iau, cu);
            D1 jvx(0.f), jvy(0.f), jdx(0.f), jdy(0.f), damp(0.f);
#pragma unroll
            for (int j = 0; j < P; ++j) {
                jvx = jvx + upx.d[j] * v[j], jvy = jvy + upy.d[j] * v[j];
                jdx = jdx + upx.d[j] * dl[j], jdy = jdy + upy.d[j] * dl[j];
                damp = damp + (upx.d[j] * upx.d[j] + upy.d[j] * upy.d[j]) * lmvd[j];
            }
            const D1 rest = jvx * jdx + jvy * jdy + damp;            // phi = jv . psi - w rest
            phi = phi + jvx * h.psi[0] + jvy * h.psi[1] - h.w * rest;
            if (k == 0 && in) {
                const float jv[2] = {jvx.v, jvy.v};
                if (a.g_up) {
                    float* gx = a.g_up + o + (size_t)b * hw;
                    const float tx = psi_grad<2>(h, r, jv, cu, 0) - h.drho * r[0].v * rest.v;
                    const float ty = psi_grad<2>(h, r, jv, cu, 1) - h.drho * r[1].v * rest.v;
                    gx[0] = store ? tx : gx[0] + tx;
                    gx[hw] = store ? ty : gx[hw] + ty;
                }
                if (a.g_upc) {
                    const float t = (jvx.v * r[0].v + jvy.v * r[1].v - rest.v) * h.rho1;
                    a.g_upc[o] = store ? t : a.g_upc[o] + t;
                }
            }
        }
        {
            const D1 r[1] = {slat - sl.v};
            const Weighted<1> h = huber_weighted<1>(r, ial, cl);
            D1 jv(0.f), jd(0.f), damp(0.f);
#pragma unroll
            for (int j = 0; j < P; ++j) {
                jv = jv + sl.d[j] * v[j];
                jd = jd + sl.d[j] * dl[j];
                damp = damp + (sl.d[j] * sl.d[j]) * lmvd[j];
            }
            const D1 rest = jv * jd + damp;
            phi = phi + jv * h.psi[0] - h.w * rest;
            if (k == 0 && in) {
                const float jvv[1] = {jv.v};
                if (a.g_lat) {
                    const float t = cosf(dlat) * (psi_grad<1>(h, r, jvv, cl, 0) - h.drho * r[0].v * rest.v);
                    a.g_lat[o] = store ? t : a.g_lat[o] + t;
                }
                if (a.g_latc) {
                    const float t = (jv.v * r[0].v - rest.v) * h.rho1;
                    a.g_latc[o] = store ? t : a.g_latc[o] + t;
                }
            }
        }
        double t = in ? (double)phi.d[0] : 0.0;
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) t += __shfl_xor(t, sh, 64);      // wave_sum's butterfly, in float64
#pragma unroll
        for (int q = 0; q < kAdj; ++q) sum[q] = q == k ? t : sum[q];
    }
    tile_record(s_sum, wave, sum, [&](int q, double s) { a.rec[((size_t)b * a.tiles + blockIdx.x) * kAdjStride + q] = s; });
}

// One block per image: word q of the image's tile records summed by 32 chains (record t goes to chain t % 32), the chains
// added in order, in float64; plus the direct term.  The adjoint of the state the step started from.
template <int MODEL>
__global__ __launch_bounds__(kBlock) void lm_grad_finish_kernel(const GradCall a, int step) {
    constexpr int kChains = kBlock / kAdjStride;
    __shared__ double part[kChains][kAdjStride];
    if (step >= last_step(a) || step == 0) return;
    const int b = blockIdx.x, q = threadIdx.x & (kAdjStride - 1), chain = threadIdx.x / kAdjStride;
    double acc = 0.0;
    if (q < state_words<MODEL>()) acc = chain_sum<kChains>(a.rec + (size_t)b * a.tiles * kAdjStride + q, kAdjStride, a.tiles, chain);
    part[chain][q] = acc;
    __syncthreads();
    if (threadIdx.x < kAdj) {
        a.adj[(size_t)b * kAdjStride + threadIdx.x] = (float)(column_sum(part, threadIdx.x) + (double)a.direct[(size_t)b * kAdjStride + threadIdx.x]);
    }
}

// workspace: adjoint, direct term, step constants, parameter jets (per image), tile records
struct Workspace {
    size_t adj, direct, stepc, params, rec, bytes;
};
Workspace workspace_of(int B, int H, int W) {
    Workspace w;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    w.adj = take((size_t)B * kAdjStride * sizeof(float));
    w.direct = take((size_t)B * kAdjStride * sizeof(float));
    w.stepc = take((size_t)B * kStepWords * sizeof(float));
    w.params = take((size_t)B * kParamFloats * sizeof(float));
    w.rec = take(tile_record_bytes(B, H, W, kAdjStride, sizeof(double)));
    w.bytes = o;
    return w;
}

}  // namespace

size_t lm_backward_workspace(int B, int H, int W) {
    return call_sizes_fit(B, H, W) ? workspace_of(B, H, W).bytes : 0;
}

hipError_t launch_lm_backward(int camera_model, const float* up, const float* lat, const float* upc, const float* latc, int B, int H,
                              int W, const float* record, int num_steps, int early_stop, const float* info, float up_scale,
                              float lat_scale, int eg, int ef, int ed, const float* grad_cam, const float* grad_grav, float* g_up,
                              float* g_lat, float* g_upc, float* g_latc, void* workspace, hipStream_t st) {
    const Workspace w = workspace_of(B, H, W);
    char* base = static_cast<char*>(workspace);
    auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    GradCall a{up, lat, up ? upc : nullptr, latc, record, info, grad_cam, grad_grav, g_up, g_lat, g_upc, g_latc,
               at(w.adj), at(w.direct), at(w.stepc), at(w.params), reinterpret_cast<double*>(base + w.rec), B, H, W, tile_columns(W, 1), tile_count(H, W, 1),
               num_steps, early_stop, eg, ef, ed, up_scale, lat_scale};
    auto run = [&](auto m) {
        constexpr int M = decltype(m)::value;
        for (int step = num_steps - 1; step >= 0; --step) {
            hipLaunchKernelGGL(lm_grad_prepare_kernel<M>, dim3((B + 63) / 64), dim3(64), 0, st, a, step);
            hipLaunchKernelGGL(lm_grad_pixel_kernel<M>, dim3(a.tiles, B), dim3(kBlock), 0, st, a, step);
            if (step > 0) hipLaunchKernelGGL(lm_grad_finish_kernel<M>, dim3(B), dim3(kBlock), 0, st, a, step);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    if (camera_model == GCLM_PINHOLE) return run(std::integral_constant<int, GCLM_PINHOLE>{});
    if (camera_model == GCLM_SIMPLE_RADIAL) return run(std::integral_constant<int, GCLM_SIMPLE_RADIAL>{});
    return hipErrorInvalidValue;
}

}  // namespace gclm
