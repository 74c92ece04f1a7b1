// gclm_field_param_grad.hip -- gclm_field_loss_param_grad / gclm_perspective_fields_backward: the gradients of the decoders'
// losses, or of any function of the rendered fields, with respect to the camera and the gravity the target fields are
// taken at (the reference gets them from autograd through get_perspective_field: both fields rendered to memory, a dozen
// eager kernels replayed backwards).  include/gclm.h: gclm_field_loss_param_grad has the mathematics.
//
// Per pixel a lane
//   - evaluates the target by the renderer's formulas (gclm_render.h: persp_row, persp_up, persp_lat) in FLOAT64 from the
//     float32 camera and gravity, the branch conditions of distort_scale / undistort_scale taken on the renderer's own
//     float32 u, r2 (gclm_field_loss.h: lane_row).  Not with the float32 functions themselves: a float32 target is 1e-7 off,
//     which is 1e-5 of a typical residual p - t and enters every cotangent that is proportional to the residual (l2, cauchy,
//     huber inside delta); over an image that does not average out below the gate of tests/field_calib_grad_gate.py (a CPU
//     restatement with the float32 target: 26 of 1080 entries above 4 units, worst 8.7; with the float64 target: worst 0.63),
//   - forms the cotangent (g_ux, g_uy, g_lat) of the target: from the loss (scale[b, field] conf dl/dt_c, the planes and loss
//     ids of gclm_field_loss_grad; dl/dt_c = -dl/dp_c by gclm_field_loss.h's pixel_grad on the rounded float64 residual, and
//     2 t_c - p_c for dot), or read from cotangent planes in the renderer's output layout (up (B, H, W, 2) interleaved,
//     latitude (B, H, W)) -- a kernel argument every lane takes alike,
//   - pulls it back through the formulas by a hand-written reverse sweep in float64: to p = (a - c u, b - c v), s, s' and
//     (u, v) for the up field; to X = u t, Y = v t, t and the gravity for the latitude; from s, s', t to r2, k1, k2 by the
//     partial derivatives of distort_scale / undistort_scale's forms (distort_partials, undistort_partials below); from r2
//     to (u, v); from (u, v) to fx, fy, cx, cy.  The derivative is that of the branch the renderer takes, the branch
//     conditions constants: 0 beyond the latitude's clamp, a constant norm below F.normalize's 1e-12, simple_divisional's
//     s = 1, s' = 0 at k1 r2 = 0.
// The terms of one parameter cancel across the image, so a lane sums in float64: eight sums (a, b, c, sum u-bar u, sum u-bar,
// sum v-bar, k1, k2), from which the row's constants give the nine of the record (a, b, c, fx, fy, cx, cy, k1, k2); wave
// (wave_sum's butterfly, written out on doubles), block (tile_record): one float64 record per tile.
// field_param_grad_finish_kernel (grid = B) sums an image's records in 16 strided chains in a fixed order and writes
// grad_cam (B, 8) -- columns w, h zero, and the distortion columns the model's formulas never read -- and grad_grav (B, 3).
// No atomics, no memset: an image's bits depend on that image, H, W and the pixels per lane alone.  64-bit offsets.  No scratch.
#include "gclm_field_loss.h"

namespace gclm {
namespace {

constexpr int kGradWords = 9;                // float64 sums per record: a, b, c, fx, fy, cx, cy, k1, k2
constexpr int kGradSlots = 16;               // threads per chain of the finish kernel (the first kGradWords work)
constexpr int kGradChains = kBlock / kGradSlots;
constexpr int kGradMaxPx = 2;                // pixels per lane: 1 or 2.  Four were measured and dropped: at 126-164 VGPRs they gain 5 % on
                                             // pinhole and lose 3-12 % on simple_divisional against two
enum { kFromLoss = 0, kFromPlanes = 1 };     // where the cotangent of the target comes from

struct ParamGradArgs {
    // from the loss: up (B, 2, H, W) / lat (B, 1, H, W) the predictions, upc / latc their confidences, scale (B, 2);
    // from planes: up (B, H, W, 2) / lat (B, H, W) the cotangents themselves
    const float *cam, *grav, *up, *lat, *upc, *latc, *scale;
    double* rec;
    int H, W, tiles_x, up_loss, lat_loss, source, normalize;
};

// A lane's sums.  uu = sum u-bar u, su = sum u-bar, sv = sum v-bar: fx, cx, fy, cy follow from them per row.
struct LaneSums {
    double a = 0.0, b = 0.0, c = 0.0, uu = 0.0, su = 0.0, sv = 0.0, k1 = 0.0, k2 = 0.0;
};

// s, s' of distort_scale and their partial derivatives, of the branch distort_scale takes (its float32 conditions):
//   simple_radial      s = 1 + k1 r2, s' = k1:                 s_r2 = k1, s_k1 = r2, s'_k1 = 1
//   radial             s = 1 + k1 r2 + k2 r2^2, s' = k1 + 2 k2 r2:  s_r2 = s', s_k1 = r2, s_k2 = r2^2, s'_r2 = 2 k2, s'_k1 = 1, s'_k2 = 2 r2
//   simple_divisional  tau = 1 - 4 k1 r2, rt = sqrt(tau), d = 1 + rt, E = rt d^2:  s = 2 / d, s' = 4 k1 / E;
//                      ds/dtau = -1 / E, so s_r2 = 4 k1 / E, s_k1 = 4 r2 / E;  dE/dtau = d (1 + 3 rt) / (2 rt), so
//                      s'_k1 = 4 / E + 16 k1 r2 E_tau / E^2,  s'_r2 = 16 k1^2 E_tau / E^2.
//                      tau < 1e-6: s' is the reference's clamped expression n / m, n = 2 k1 r2 - (1 - tt) tt, m = 2 k1 r2^2 tt,
//                      tt = 1e-3:  s'_k1 = (2 r2 m - n 2 r2^2 tt) / m^2,  s'_r2 = (2 k1 m - n 4 k1 r2 tt) / m^2;
//                      tau <= 0: s = 1 / (2 k1 r2):  s_k1 = -s / k1, s_r2 = -s / r2;  k1 r2 = 0: constants, every partial 0.
struct DistortPartials {
    double s, sp, s_r2, s_k1, s_k2, sp_r2, sp_k1, sp_k2;
};
template <int MODEL>
__device__ __forceinline__ DistortPartials distort_partials(double r2, float r2f, float k1f, float k2f) {
    const double k1 = k1f, k2 = k2f;
    DistortPartials o{1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (MODEL == GCLM_SIMPLE_RADIAL) {
        o.s = 1.0 + k1 * r2, o.sp = k1;
        o.s_r2 = k1, o.s_k1 = r2, o.sp_k1 = 1.0;
    } else if constexpr (MODEL == GCLM_RADIAL) {
        o.s = 1.0 + (k1 + k2 * r2) * r2, o.sp = k1 + 2.0 * k2 * r2;
        o.s_r2 = o.sp, o.s_k1 = r2, o.s_k2 = r2 * r2;
        o.sp_r2 = 2.0 * k2, o.sp_k1 = 1.0, o.sp_k2 = 2.0 * r2;
    } else if constexpr (MODEL == GCLM_SIMPLE_DIVISIONAL) {
        const float krf = k1f * r2f, tauf = 1.f - 4.f * krf;          // the conditions as distort_scale evaluates them
        if (krf == 0.f) return o;
        // (tau in float64 where the float32 value is clear of 0, else the float32 value itself: the two differ by a few 1e-7,
        // and a float64 tau <= 0 under a float32 tau > 0 would divide by sqrt(0))
        const double kr = k1 * r2, tau = tauf >= 1e-6f || tauf <= 0.f ? 1.0 - 4.0 * kr : (double)tauf;
        if (tauf > 0.f) {
            const double rt = sqrt(tau), d = 1.0 + rt, iE = 1.0 / (rt * d * d);
            o.s = 2.0 / d;
            o.s_r2 = 4.0 * k1 * iE, o.s_k1 = 4.0 * r2 * iE;
            if (tauf >= 1e-6f) {
                const double w = 16.0 * k1 * (d * (1.0 + 3.0 * rt) / (2.0 * rt)) * iE * iE;
                o.sp = o.s_r2;
                o.sp_k1 = 4.0 * iE + w * r2, o.sp_r2 = w * k1;
            }
        } else {
            o.s = 1.0 / (2.0 * kr);
            o.s_k1 = -o.s / k1, o.s_r2 = -o.s / r2;
        }
        if (!(tauf >= 1e-6f)) {
            const double tt = (double)sqrtf(1e-6f), n = 2.0 * kr - (1.0 - tt) * tt, m = 2.0 * k1 * (r2 * r2) * tt;
            if (m != 0.0) {
                o.sp = n / m;
                o.sp_k1 = (2.0 * r2 * m - n * 2.0 * (r2 * r2) * tt) / (m * m);
                o.sp_r2 = (2.0 * k1 * m - n * 4.0 * kr * tt) / (m * m);
            } else {
                o.sp = n / 1e6;
            }
        }
    }
    return o;
}

// t of undistort_scale and its partial derivatives: simple_radial t = 1 - k1 r2; radial t = 1 - k1 r2 + (3 k1^2 - k2) r2^2;
// simple_divisional t = 1 / (1 + k1 r2): t_r2 = -k1 t^2, t_k1 = -r2 t^2 (a zero denominator: the constant 1e-6).
struct UndistortPartials {
    double t, t_r2, t_k1, t_k2;
};
template <int MODEL>
__device__ __forceinline__ UndistortPartials undistort_partials(double r2, float r2f, float k1f, float k2f) {
    const double k1 = k1f, k2 = k2f;
    UndistortPartials o{1.0, 0.0, 0.0, 0.0};
    if constexpr (MODEL == GCLM_SIMPLE_RADIAL) {
        o.t = 1.0 - k1 * r2;
        o.t_r2 = -k1, o.t_k1 = -r2;
    } else if constexpr (MODEL == GCLM_RADIAL) {
        const double q = 3.0 * k1 * k1 - k2;
        o.t = 1.0 - k1 * r2 + q * (r2 * r2);
        o.t_r2 = -k1 + 2.0 * q * r2, o.t_k1 = -r2 + 6.0 * k1 * (r2 * r2), o.t_k2 = -(r2 * r2);
    } else if constexpr (MODEL == GCLM_SIMPLE_DIVISIONAL) {
        if (1.f + k1f * r2f == 0.f) {
            o.t = 1e-6;
        } else {
            o.t = 1.0 / (1.0 + k1 * r2);
            o.t_r2 = -k1 * o.t * o.t, o.t_k1 = -r2 * o.t * o.t;
        }
    }
    return o;
}

// The image's and the row's terms in float64, from the float32 entries persp_row reads.
struct Row64 {
    double ifx, ify, cx, a, b, c, v;
    float k1, k2;
};
__device__ __forceinline__ Row64 row64(const float* cb, const float* gb, int y) {
    Row64 r;
    r.ifx = 1.0 / (double)cb[2], r.ify = 1.0 / (double)cb[3];
    r.cx = cb[4], r.k1 = cb[6], r.k2 = cb[7];
    r.a = gb[0], r.b = gb[1], r.c = gb[2];
    r.v = ((double)y - (double)cb[5]) * r.ify;
    return r;
}

// The up field of one pixel (persp_up's formulas, in float64): the terms the reverse sweep reads, and the field itself.
struct UpPixel {
    double px, py, dot, o, in, tx, ty;         // in = 1 / max(|q|, 1e-12), or 1 without normalisation; t = q in
    bool floor;                                // F.normalize's clamp_min acts: a constant norm
    DistortPartials d;
};
template <int MODEL>
__device__ __forceinline__ UpPixel up_forward(const Row64& r, double u, double r2, float r2f, bool normalize) {
    UpPixel f;
    f.px = r.a - r.c * u, f.py = r.b - r.c * r.v;
    f.dot = 0.0, f.o = 0.0;
    f.d = DistortPartials{1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double qx = f.px, qy = f.py;
    if constexpr (MODEL != GCLM_PINHOLE) {
        f.d = distort_partials<MODEL>(r2, r2f, r.k1, r.k2);
        f.dot = u * f.px + r.v * f.py;
        f.o = 2.0 * f.d.sp * f.dot;
        qx = f.d.s * f.px + f.o * u;
        qy = f.d.s * f.py + f.o * r.v;
    }
    f.in = 1.0, f.floor = false;
    if (normalize) {
        const double n = sqrt(qx * qx + qy * qy);
        f.floor = n < 1e-12;                        // (a NaN norm stays NaN)
        f.in = f.floor ? 1e12 : 1.0 / n;
    }
    f.tx = qx * f.in, f.ty = qy * f.in;
    return f;
}

// ... and its cotangent (gx, gy) pulled back.
template <int MODEL>
__device__ __forceinline__ void pull_up(const Row64& r, const UpPixel& f, double u, bool normalize, double gx, double gy, LaneSums& acc) {
    if (normalize) {
        const double along = f.floor ? 0.0 : f.tx * gx + f.ty * gy;
        gx = (gx - f.tx * along) * f.in;
        gy = (gy - f.ty * along) * f.in;
    }
    double pbx = gx, pby = gy, ub = 0.0, vb = 0.0;
    if constexpr (MODEL != GCLM_PINHOLE) {
        const DistortPartials& d = f.d;
        const double sb = gx * f.px + gy * f.py, ob = gx * u + gy * r.v;
        const double spb = 2.0 * f.dot * ob, db = 2.0 * d.sp * ob;
        pbx = d.s * gx + db * u, pby = d.s * gy + db * r.v;
        const double r2b = sb * d.s_r2 + spb * d.sp_r2;
        ub = f.o * gx + db * f.px + 2.0 * u * r2b;
        vb = f.o * gy + db * f.py + 2.0 * r.v * r2b;
        acc.k1 += sb * d.s_k1 + spb * d.sp_k1;
        if constexpr (MODEL == GCLM_RADIAL) acc.k2 += sb * d.s_k2 + spb * d.sp_k2;
    }
    ub -= pbx * r.c, vb -= pby * r.c;
    acc.a += pbx, acc.b += pby, acc.c -= pbx * u + pby * r.v;
    acc.uu += ub * u, acc.su += ub, acc.sv += vb;
}

// The latitude of one pixel (persp_lat's formulas, in float64): sl is the sine before the clamp.
struct LatPixel {
    double X, Y, in, sl;
    UndistortPartials d;
};
template <int MODEL>
__device__ __forceinline__ LatPixel lat_forward(const Row64& r, double u, double r2, float r2f) {
    LatPixel f;
    f.d = undistort_partials<MODEL>(r2, r2f, r.k1, r.k2);
    f.X = u * f.d.t, f.Y = r.v * f.d.t;
    f.in = 1.0 / sqrt(f.X * f.X + f.Y * f.Y + 1.0);
    f.sl = (f.X * r.a + f.Y * r.b + r.c) * f.in;
    return f;
}
__device__ __forceinline__ double latitude(const LatPixel& f) {
    const double hi = (double)kLatHi;
    return asin(f.sl < -hi ? -hi : (f.sl > hi ? hi : f.sl));          // a NaN stays NaN
}

// ... and its cotangent g pulled back.
template <int MODEL>
__device__ __forceinline__ void pull_lat(const Row64& r, const LatPixel& f, double u, double g, LaneSums& acc) {
    const double sl = f.sl, in = f.in;
    if (sl < -(double)kLatHi || sl > (double)kLatHi) return;          // the clamp: a constant beyond it (a NaN goes on: NaN)
    const double sb = g / sqrt((1.0 - sl) * (1.0 + sl));
    const double Xb = sb * (r.a - sl * f.X * in) * in, Yb = sb * (r.b - sl * f.Y * in) * in;
    double ub = Xb * f.d.t, vb = Yb * f.d.t;
    if constexpr (MODEL != GCLM_PINHOLE) {
        const double tb = Xb * u + Yb * r.v, r2b = tb * f.d.t_r2;
        ub += 2.0 * u * r2b, vb += 2.0 * r.v * r2b;
        acc.k1 += tb * f.d.t_k1;
        if constexpr (MODEL == GCLM_RADIAL) acc.k2 += tb * f.d.t_k2;
    }
    acc.a += sb * f.X * in, acc.b += sb * f.Y * in, acc.c += sb * in;
    acc.uu += ub * u, acc.su += ub, acc.sv += vb;
}

// A lane's PX adjacent cotangents of the interleaved up plane: p points at (x, y)'s pair.
template <int PX>
__device__ __forceinline__ void load_pairs(const float* __restrict__ p, float (&gx)[PX], float (&gy)[PX]) {
    static_assert(PX == 1 || PX == 2, "one pair is a dwordx2, two are a dwordx4");
    if constexpr (PX == 1) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(p);
        gx[0] = t.x, gy[0] = t.y;
    } else {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        gx[0] = t.x, gy[0] = t.y, gx[1] = t.z, gy[1] = t.w;
    }
}

template <int MODEL, int PX>
__global__ __launch_bounds__(kBlock) void field_param_grad_kernel(const ParamGradArgs a) {
    __shared__ double s_sum[kTileRows][kGradWords];
    int x, y;
    const bool in = tile_pixel<PX>(a.tiles_x, a.H, a.W, x, y);
    const int b = blockIdx.y, wave = threadIdx.x >> 6;
    double sum[kGradWords] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (in) {
        float uf[PX], r2f[PX];                     // the renderer's float32 u, r2: its branch conditions are taken on them
        lane_row<PX>(a.cam, a.grav, b, x, y, uf, r2f);
        const Row64 r = row64(a.cam + (size_t)b * 8, a.grav + (size_t)b * 3, y);
        const size_t hw = (size_t)a.H * a.W, o = (size_t)b * hw + (size_t)y * a.W + x;
        const bool loss = a.source == kFromLoss, nrm = loss || a.normalize != 0;
        LaneSums acc;
        if (a.up) {
            float p0[PX], p1[PX], c[PX];           // from the loss: prediction and confidence; from planes: the cotangent itself
            if (loss) {
                load_px<PX>(a.up + o + (size_t)b * hw, p0);          // (B, 2, H, W): image b starts at 2 b H W
                load_px<PX>(a.up + o + (size_t)b * hw + hw, p1);
                if (a.upc) load_px<PX>(a.upc + o, c);
            } else {
                load_pairs<PX>(a.up + 2 * o, p0, p1);
            }
            const double scale = loss ? (double)a.scale[(size_t)b * 2] : 1.0;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const double u = ((double)(x + j) - r.cx) * r.ifx, r2 = u * u + r.v * r.v;
                const UpPixel f = up_forward<MODEL>(r, u, r2, r2f[j], nrm);
                double gx = p0[j], gy = p1[j];
                if (loss) {
                    const double rx = (double)p0[j] - f.tx, ry = (double)p1[j] - f.ty;
                    if (a.up_loss == GCLM_FIELD_LOSS_DOT) {           // l = 1 - sum (p - t) t:  dl/dt_c = t_c - r_c = 2 t_c - p_c
                        gx = f.tx - rx, gy = f.ty - ry;
                    } else {                                          // l = l(p - t):  dl/dt_c = -dl/dp_c
                        const float rr[2] = {(float)rx, (float)ry}, tt[2] = {(float)f.tx, (float)f.ty};
                        float g[2];
                        pixel_grad<2>(a.up_loss, rr, tt, g);
                        gx = -(double)g[0], gy = -(double)g[1];
                    }
                    const double w = a.upc ? scale * (double)c[j] : scale;
                    gx *= w, gy *= w;
                }
                pull_up<MODEL>(r, f, u, nrm, gx, gy, acc);
            }
        }
        if (a.lat) {
            float p[PX], c[PX];
            load_px<PX>(a.lat + o, p);
            if (loss && a.latc) load_px<PX>(a.latc + o, c);
            const double scale = loss ? (double)a.scale[(size_t)b * 2 + 1] : 1.0;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const double u = ((double)(x + j) - r.cx) * r.ifx, r2 = u * u + r.v * r.v;
                const LatPixel f = lat_forward<MODEL>(r, u, r2, r2f[j]);
                double g = p[j];
                if (loss) {
                    const float rr[1] = {(float)((double)p[j] - latitude(f))}, tt[1] = {0.f};
                    float gp[1];
                    pixel_grad<1>(a.lat_loss, rr, tt, gp);           // (never dot: tt is not read)
                    g = -(double)gp[0] * (a.latc ? scale * (double)c[j] : scale);
                }
                pull_lat<MODEL>(r, f, u, g, acc);
            }
        }
        // u = (x - cx) / fx, v = (y - cy) / fy:  du/dfx = -u / fx, du/dcx = -1 / fx, and likewise for v
        sum[0] = acc.a, sum[1] = acc.b, sum[2] = acc.c;
        sum[3] = -acc.uu * r.ifx, sum[4] = -acc.sv * r.v * r.ify;
        sum[5] = -acc.su * r.ifx, sum[6] = -acc.sv * r.ify;
        sum[7] = acc.k1, sum[8] = acc.k2;
    }
    // every lane of the block from here on: wave sums (wave_sum's butterfly, in float64), one record per tile
#pragma unroll
    for (int k = 0; k < kGradWords; ++k) {
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) sum[k] += __shfl_xor(sum[k], sh, 64);
    }
    tile_record(s_sum, wave, sum, [&](int k, double s) { a.rec[((size_t)b * gridDim.x + blockIdx.x) * kGradWords + k] = s; });
}

// One block per image: word k of the image's tile records summed by kGradChains chains (record t goes to chain
// t % kGradChains), the chains added in order, in float64.  grad_cam (B, 8): w, h zero, fx, fy, cx, cy, k1, k2 -- k2 zero for
// the one-parameter models, both zero for pinhole; grad_grav (B, 3).  Either may be NULL.
__global__ __launch_bounds__(kBlock) void field_param_grad_finish_kernel(const double* __restrict__ rec, int tiles, int model,
                                                                         float* __restrict__ grad_cam, float* __restrict__ grad_grav) {
    __shared__ double part[kGradChains][kGradSlots];
    const int b = blockIdx.x, k = threadIdx.x & (kGradSlots - 1), chain = threadIdx.x / kGradSlots;
    part[chain][k] = k < kGradWords ? chain_sum<kGradChains>(rec + (size_t)b * tiles * kGradWords + k, kGradWords, tiles, chain) : 0.0;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 8 && grad_cam) {
        const int dist = model == GCLM_PINHOLE ? 0 : (model == GCLM_RADIAL ? 2 : 1);
        grad_cam[(size_t)b * 8 + t] = (t >= 2 && t < 6 + dist) ? (float)column_sum(part, t + 1) : 0.f;
    }
    if (t >= 8 && t < 11 && grad_grav) grad_grav[(size_t)b * 3 + (t - 8)] = (float)column_sum(part, t - 8);
}

hipError_t launch_param_grad(int camera_model, const ParamGradArgs& args, int B, int px, float* grad_cam, float* grad_grav, hipStream_t st) {
    ParamGradArgs a = args;
    a.tiles_x = tile_columns(a.W, px);
    const int tiles = tile_count(a.H, a.W, px);
    return with_camera_model(camera_model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const auto kernel = with_pixels_per_lane<kGradMaxPx>(px, [](auto p) { return field_param_grad_kernel<M, decltype(p)::value>; });
        hipLaunchKernelGGL(kernel, dim3(tiles, B), dim3(kBlock), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(field_param_grad_finish_kernel, dim3(B), dim3(kBlock), 0, st, static_cast<const double*>(a.rec), tiles,
                           camera_model, grad_cam, grad_grav);
        return hipGetLastError();
    });
}

}  // namespace

size_t field_param_grad_workspace(int B, int H, int W) {
    return call_sizes_fit(B, H, W) ? tile_record_bytes(B, H, W, kGradWords, sizeof(double)) : 0;
}

hipError_t launch_field_loss_param_grad(int camera_model, const float* cam, const float* grav, int B, int H, int W, const float* up,
                                        const float* lat, const float* upc, const float* latc, int up_loss, int lat_loss,
                                        const float* scale, void* workspace, float* grad_cam, float* grad_grav, hipStream_t st) {
    const int px = pixels_per_lane(W, {up, lat, upc, latc}, kGradMaxPx);
    const ParamGradArgs a{cam, grav, up, lat, upc, latc, scale, static_cast<double*>(workspace), H, W, 0, up_loss, lat_loss, kFromLoss, 1};
    return launch_param_grad(camera_model, a, B, px, grad_cam, grad_grav, st);
}

hipError_t launch_perspective_fields_backward(int camera_model, const float* cam, const float* grav, int B, int H, int W, int normalize,
                                              const float* grad_up, const float* grad_lat, void* workspace, float* grad_cam,
                                              float* grad_grav, hipStream_t st) {
    // a lane's pixels are 2 PX floats of the interleaved up plane: that plane is held to twice the alignment
    int px = pixels_per_lane(W, {grad_lat}, kGradMaxPx);
    while (px > 1 && reinterpret_cast<uintptr_t>(grad_up) % (8 * (size_t)px) != 0) px /= 2;
    const ParamGradArgs a{cam, grav, grad_up, grad_lat, nullptr, nullptr, nullptr, static_cast<double*>(workspace), H, W, 0, 0, 0,
                          kFromPlanes, normalize};
    return launch_param_grad(camera_model, a, B, px, grad_cam, grad_grav, st);
}

}  // namespace gclm
