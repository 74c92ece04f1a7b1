// gclm_entry.hip -- the entry points of include/gclm.h that take no handle: the stage kernels, the head epilogue and the
// upsampler, the five render kernels, the field errors, the field losses and their gradients (to the fields, and to the camera and gravity), the classification heads' loss and its gradient, the adjoint of the LM steps, the hypothesis scores, the minimal solver, the Adam optimiser on (roll, pitch, vfov), the synthetic fields and the read probe.  Each checks its arguments
// before the first HIP call -- plain conditions first, then the ranges the call writes and reads over the one checker,
// gclm_args.h -- and launches on the caller's stream and current device.  Host code only: this unit holds no kernel.
#include <cfloat>
#include <cmath>

#include "gclm_args.h"
#include "gclm_render.h"

using namespace gclm;

namespace {
int launched(hipError_t e) { return e == hipSuccess ? 0 : -10; }

// The two image warps, for float32 (T = float) and byte (T = unsigned char) images alike.  `interleaved` is the byte calls'
// layout flag -- an interleaved image has at most 4 channels -- and the float calls pass 0, so neither its refusal nor the
// dword path can reach them.  The dword path of C = 4 is taken where both images allow it (the same bytes either way).
// Undistort states no alignment and no camera range; reproject holds an image to its element's alignment.
template <typename T>
int undistort_image(int camera_model, const float* d_cam, int cam_batch, const T* d_src, int B, int C, int Hin, int Win, int H, int W,
                    int interleaved, T* d_dst, void* stream) {
    if (!d_cam || !d_src || !d_dst || B < 1 || B > kMaxCallImages || C < 1 || Hin < 1 || Win < 1 || H < 2 || W < 2) return -3;
    if ((cam_batch != 1 && cam_batch != B) || !known_model(camera_model) || (int64_t)H * W > INT32_MAX) return -3;
    if ((interleaved != 0 && interleaved != 1) || (interleaved && C > 4)) return -3;
    ArgCheck a;
    a.writes(d_dst, elements<T>(B, C, H, W));
    a.reads(d_src, elements<T>(B, C, Hin, Win));
    if (!a.pass()) return -3;
    const bool dwords = interleaved && C == 4 && is_aligned(d_src, 4) && is_aligned(d_dst, 4);
    return launched(launch_undistort_image(camera_model, d_cam, cam_batch, d_src, B, C, Hin, Win, H, W, interleaved != 0, dwords,
                                           d_dst, static_cast<hipStream_t>(stream)));
}

template <typename T>
int reproject_image(int src_model, const float* d_src_cam, int dst_model, const float* d_dst_cam, int cam_batch, const float* d_rot,
                    int rot_batch, const T* d_src, int B, int C, int Hin, int Win, int Hs, int Ws, int H, int W, int interleaved,
                    T* d_dst, unsigned char* d_valid, void* stream) {
    if (!d_src_cam || !d_dst_cam || !d_src || !d_dst || B < 1 || B > kMaxCallImages || C < 1 || Hin < 1 || Win < 1) return -3;
    if (H < 1 || W < 1 || Hs < 2 || Ws < 2 || !tile_grid_fits(H, W) || !known_model(src_model) || !known_model(dst_model)) return -3;
    if ((cam_batch != 1 && cam_batch != B) || (rot_batch != 1 && rot_batch != B)) return -3;
    if ((interleaved != 0 && interleaved != 1) || (interleaved && C > 4)) return -3;
    ArgCheck a;
    a.writes(d_dst, elements<T>(B, C, H, W), alignof(T));
    a.writes(d_valid, elements<unsigned char>(B, H, W));
    a.reads(d_src_cam, floats(cam_batch, 8), 4);
    a.reads(d_dst_cam, floats(cam_batch, 8), 4);
    a.reads(d_rot, floats(rot_batch, 9), 4);
    a.reads(d_src, elements<T>(B, C, Hin, Win), alignof(T));
    if (!a.pass()) return -3;
    const bool dwords = interleaved && C == 4 && is_aligned(d_src, 4) && is_aligned(d_dst, 4);
    return launched(launch_reproject_image(src_model, d_src_cam, dst_model, d_dst_cam, cam_batch, d_rot, rot_batch, d_src, B, C, Hin,
                                           Win, Hs, Ws, H, W, interleaved != 0, dwords, d_dst, d_valid,
                                           static_cast<hipStream_t>(stream)));
}

// gclm_draw_fields / gclm_draw_fields_u8: the one check of both, plain conditions first (the style among them), then the
// ranges.  The arrow geometry is held to its conditions only where the arrow layer is on: the demo's defaults violate the
// reach condition on portrait frames, and a caller who draws no arrows must not be refused for them.
constexpr uint32_t kOverlayLayers = GCLM_OVERLAY_HEAT | GCLM_OVERLAY_TINT | GCLM_OVERLAY_CONTOURS | GCLM_OVERLAY_HORIZON | GCLM_OVERLAY_ARROWS;
bool unit_interval(float v) { return v >= 0.f && v <= 1.f; }                 // (false for NaN)
bool finite_nonneg(float v) { return v >= 0.f && v <= FLT_MAX; }

// gclm_param_opt / gclm_param_opt_step: the one check of a config (include/gclm.h lists the conditions)
bool finite_nonneg(double v) { return v >= 0.0 && v <= DBL_MAX; }
bool param_opt_config_ok(const gclm_param_opt_config& c) {
    if (c.struct_size != (int32_t)sizeof(gclm_param_opt_config) || c.max_steps < 1 || c.max_steps > GCLM_PARAM_OPT_MAX_STEPS) return false;
    if (c.patience < 1 || c.patience > GCLM_PARAM_OPT_MAX_PATIENCE || c.sched_patience < 0 || c.sched_cooldown < 0 || c.poll_every < 0)
        return false;
    if (!finite_nonneg(c.lr) || !(c.lamb >= 0.0 && c.lamb <= 1.0) || c.abs_tol != c.abs_tol || c.rel_tol != c.rel_tol) return false;
    return c.sched_factor >= 0.0 && c.sched_factor < 1.0 && finite_nonneg(c.sched_threshold) && finite_nonneg(c.sched_min_lr) &&
           finite_nonneg(c.sched_eps);
}

template <typename T>
int draw_fields(int camera_model, const float* d_cam, const float* d_grav, int cal_batch, const T* d_src, int B, int C, int H, int W,
                int interleaved, const float* d_conf, const unsigned char* d_palette, const unsigned char* d_heat_palette,
                const gclm_overlay_style* style, T* d_dst, void* stream) {
    if (!d_cam || !d_grav || !d_src || !d_dst || !style || !known_model(camera_model) || B < 1 || B > kMaxCallImages) return -3;
    if ((C != 3 && C != 4) || H < 1 || W < 1 || !tile_grid_fits(H, W) || (cal_batch != 1 && cal_batch != B)) return -3;
    if (interleaved != 0 && interleaved != 1) return -3;
    const gclm_overlay_style st = *style;
    if (st.struct_size != (int32_t)sizeof(gclm_overlay_style) || (st.layers & ~kOverlayLayers)) return -3;
    if (!unit_interval(st.heat_alpha) || !unit_interval(st.tint_alpha)) return -3;
    if (!(fabsf(st.heat_lo) <= FLT_MAX) || !(fabsf(st.heat_hi) <= FLT_MAX) || !(st.heat_hi > st.heat_lo)) return -3;
    if (st.levels < 2 || ((st.layers & GCLM_OVERLAY_HORIZON) && st.levels % 2 == 0)) return -3;
    if (!finite_nonneg(st.line_halfwidth) || !finite_nonneg(st.arrow_halfwidth) || !finite_nonneg(st.arrow_length)) return -3;
    if (st.layers & GCLM_OVERLAY_ARROWS) {
        if (st.arrow_step < 1 || st.arrow_x0 < 0 || st.arrow_y0 < 0 || !unit_interval(st.arrow_tip)) return -3;
        if (!((double)st.arrow_length + st.arrow_halfwidth + 0.5 <= (double)st.arrow_step)) return -3;
    }
    if ((st.layers & GCLM_OVERLAY_HEAT) && (!d_conf || !d_heat_palette)) return -3;
    if ((st.layers & (GCLM_OVERLAY_TINT | GCLM_OVERLAY_CONTOURS)) && !d_palette) return -3;
    ArgCheck a;
    a.writes(d_dst, elements<T>(B, C, H, W), alignof(T));
    a.reads(d_cam, floats(cal_batch, 8), 4);
    a.reads(d_grav, floats(cal_batch, 3), 4);
    a.reads(d_src, elements<T>(B, C, H, W), alignof(T));
    a.reads(d_conf, floats(B, H, W), 4);
    a.reads(d_palette, 768);
    a.reads(d_heat_palette, 768);
    if (!a.pass()) return -3;
    const bool dwords = interleaved && C == 4 && is_aligned(d_src, 4) && is_aligned(d_dst, 4);
    return launched(launch_draw_fields(camera_model, d_cam, d_grav, cal_batch, d_src, B, C, H, W, interleaved != 0, dwords, d_conf,
                                       d_palette, d_heat_palette, st, d_dst, static_cast<hipStream_t>(stream)));
}

// gclm_field_loss / gclm_field_loss_grad: the plain conditions the two share
bool field_loss_plain_ok(int camera_model, const float* d_cam, const float* d_grav, const float* d_up, const float* d_lat,
                         const float* d_up_conf, const float* d_lat_conf, int up_loss, int lat_loss) {
    if (!d_cam || !d_grav || (!d_up && !d_lat) || (!d_up && d_up_conf) || (!d_lat && d_lat_conf) || !known_model(camera_model)) return false;
    if (up_loss < GCLM_FIELD_LOSS_L1 || up_loss > GCLM_FIELD_LOSS_HUBER || lat_loss < GCLM_FIELD_LOSS_L1 || lat_loss > GCLM_FIELD_LOSS_HUBER)
        return false;
    return lat_loss != GCLM_FIELD_LOSS_DOT;
}

// gclm_bin_loss / gclm_bin_loss_grad: the plain conditions the two share -- at least one head, a head's count in range (an
// absent head's count is not looked at), a confidence only beside its head, a known logit type, sizes of the right sign
bool bin_loss_plain_ok(const void* d_up_logits, int up_bins, const void* d_lat_logits, int lat_bins, int logit_dtype,
                       const float* d_up_conf, const float* d_lat_conf, int B, int H, int W) {
    if ((!d_up_logits && !d_lat_logits) || (!d_up_logits && d_up_conf) || (!d_lat_logits && d_lat_conf)) return false;
    if (d_up_logits && (up_bins < 2 || up_bins > GCLM_MAX_BINS)) return false;
    if (d_lat_logits && (lat_bins < 1 || lat_bins > GCLM_MAX_BINS)) return false;
    if (logit_dtype != GCLM_LOGITS_F32 && logit_dtype != GCLM_LOGITS_F16 && logit_dtype != GCLM_LOGITS_BF16) return false;
    return B >= 0 && H >= 1 && W >= 1;
}
}  // namespace

extern "C" {

int gclm_gradient_hessian(const float* d_J, const float* d_residual, const float* d_weight, int B, int N, int R,
                          int P, int accumulate, float* d_G, float* d_H, void* stream) {
    if (!d_J || !d_residual || !d_weight || !d_G || !d_H || B < 0 || N < 0 || R < 1 || R > 4 || P < 1 ||
        P > GCLM_MAX_PARAMS)
        return -3;
    return launched(launch_gradient_hessian(d_J, d_residual, d_weight, B, N, R, P, accumulate, d_G, d_H,
                                            static_cast<hipStream_t>(stream)));
}

int gclm_optimizer_step(const float* d_G, const float* d_H, const float* d_lambda, int lambda_is_scalar, float eps,
                        int B, int P, float* d_delta, int* d_failed, void* stream) {
    if (!d_G || !d_H || !d_lambda || !d_delta || B < 0 || P < 1 || P > GCLM_MAX_PARAMS) return -3;
    return launched(launch_lm_step(d_G, d_H, d_lambda, lambda_is_scalar ? 0 : 1, eps, B, P, d_delta, d_failed,
                                   static_cast<hipStream_t>(stream)));
}

int gclm_residual_fields(int camera_model, const float* d_up, const float* d_lat, const float* d_cam,
                         const float* d_grav, int B, int H, int W, float* d_r_up, float* d_r_lat, void* stream) {
    if (!d_cam || !d_grav || (!d_r_up && !d_r_lat) || B < 0 || H <= 0 || W <= 0) return -3;
    if ((d_r_up && !d_up) || (d_r_lat && !d_lat)) return -3;
    if (!known_model(camera_model) || B > kMaxCallImages) return -3;
    return launched(launch_residual_fields(camera_model, d_up, d_lat, d_cam, d_grav, B, H, W, d_r_up, d_r_lat,
                                           static_cast<hipStream_t>(stream)));
}

int gclm_huber_costs(const float* d_residual, size_t n, int dim, float scale, const float* d_conf, float* d_cost,
                     float* d_weight, float* d_second, void* stream) {
    if (!d_residual || (!d_cost && !d_weight && !d_second) || dim < 0 || dim > 4 || !(scale > 0.f)) return -3;
    return launched(launch_huber_costs(d_residual, n, dim, scale, d_conf, d_cost, d_weight, d_second,
                                       static_cast<hipStream_t>(stream)));
}

int gclm_jacobian_fields(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W,
                         int spherical, int log_focal, float* d_J_up, float* d_J_lat, void* stream) {
    if (!d_cam || !d_grav || (!d_J_up && !d_J_lat) || B < 0 || H <= 0 || W <= 0) return -3;
    if (!known_model(camera_model) || B > kMaxCallImages) return -3;
    return launched(launch_jacobian_fields(camera_model, d_cam, d_grav, B, H, W, spherical, log_focal, d_J_up, d_J_lat,
                                           static_cast<hipStream_t>(stream)));
}

int gclm_upsample_fields(const float* d_src, int planes, int h, int w, int H, int W, float* d_dst, void* stream) {
    if (!d_src || !d_dst || planes < 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return -3;
    return launched(launch_upsample(d_src, planes, h, w, H, W, d_dst, static_cast<hipStream_t>(stream)));
}

int gclm_upsample_fields_multi(const float* const* d_srcs, float* const* d_dsts, const int* planes, int n_tensors, int h, int w,
                               int H, int W, void* stream) {
    if (!d_srcs || !d_dsts || !planes || n_tensors < 1 || n_tensors > kMaxUpsampleTensors || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return -1;
    UpsampleMulti m{};
    m.n = n_tensors;
    for (int t = 0; t < n_tensors; ++t) {
        if (planes[t] < 0 || (planes[t] > 0 && (!d_srcs[t] || !d_dsts[t]))) return -1;
        m.src[t] = d_srcs[t]; m.dst[t] = d_dsts[t]; m.planes[t] = planes[t];
    }
    return launched(launch_upsample_multi(m, h, w, H, W, static_cast<hipStream_t>(stream)));
}

int gclm_pack_fields_ex(const float* d_up_raw, const float* d_up_logconf, const float* d_lat_raw,
                        const float* d_lat_logconf, int B, int H, int W, float* d_up, float* d_up_conf, float* d_lat,
                        float* d_lat_conf, float* d_sin_lat, void* stream) {
    if (!d_up_raw || !d_lat_raw || !d_up || !d_lat || B < 0 || H <= 0 || W <= 0) return -3;
    if ((d_up_logconf && !d_up_conf) || (d_lat_logconf && !d_lat_conf)) return -3;
    // The sixth plane is written from registers but must not land on a plane the pass still reads or writes.  The other four
    // outputs are registered as if read: the sixth plane keeps off them, and they may alias the inputs (pack_fields(inplace=True)).
    // (the first two hold two planes per image)
    const float* const planes[] = {d_up_raw, d_up, d_up_logconf, d_lat_raw, d_lat_logconf, d_up_conf, d_lat, d_lat_conf};
    ArgCheck a;
    const size_t plane = floats(B, H, W);
    a.writes(d_sin_lat, plane);
    bool vec4 = ((size_t)H * W) % 4 == 0 && is_aligned(d_sin_lat, 16);
    for (int k = 0; k < 8; ++k) {
        a.reads(planes[k], mul_sat(plane, k < 2 ? 2 : 1));
        vec4 = vec4 && is_aligned(planes[k], 16);
    }
    if (!a.pass()) return -3;
    return launched(launch_pack_fields(d_up_raw, d_up_logconf, d_lat_raw, d_lat_logconf, B, H, W, vec4, d_up, d_up_conf,
                                       d_lat, d_lat_conf, d_sin_lat, static_cast<hipStream_t>(stream)));
}

int gclm_pack_fields(const float* d_up_raw, const float* d_up_logconf, const float* d_lat_raw,
                     const float* d_lat_logconf, int B, int H, int W, float* d_up, float* d_up_conf, float* d_lat,
                     float* d_lat_conf, void* stream) {
    return gclm_pack_fields_ex(d_up_raw, d_up_logconf, d_lat_raw, d_lat_logconf, B, H, W, d_up, d_up_conf, d_lat, d_lat_conf,
                               nullptr, stream);
}

int gclm_pack_fields_typed(int raw_dtype, const void* d_up_raw, const void* d_up_logconf, const void* d_lat_raw,
                           const void* d_lat_logconf, int B, int H, int W, float* d_up, float* d_up_conf, float* d_lat,
                           float* d_lat_conf, float* d_sin_lat, void* stream) {
    // float32 raws: gclm_pack_fields_ex itself -- its checks (outputs may alias their inputs), its kernel, its bits
    if (raw_dtype == GCLM_LOGITS_F32)
        return gclm_pack_fields_ex(static_cast<const float*>(d_up_raw), static_cast<const float*>(d_up_logconf),
                                   static_cast<const float*>(d_lat_raw), static_cast<const float*>(d_lat_logconf), B, H, W, d_up,
                                   d_up_conf, d_lat, d_lat_conf, d_sin_lat, stream);
    if (raw_dtype != GCLM_LOGITS_F16 && raw_dtype != GCLM_LOGITS_BF16) return -3;
    if (!d_up_raw || !d_lat_raw || !d_up || !d_lat || B < 0 || H <= 0 || W <= 0) return -3;
    if ((d_up_logconf && !d_up_conf) || (d_lat_logconf && !d_lat_conf)) return -3;
    // 16-bit raws: an output is twice its input's size, so nothing is converted in place -- every plane written keeps off
    // every other plane of the call.  A confidence output without its log-confidence is not written and names no range.
    const size_t px = floats(B, H, W), raw = elements<uint16_t>(B, H, W);
    float* const up_conf = d_up_logconf ? d_up_conf : nullptr;
    float* const lat_conf = d_lat_logconf ? d_lat_conf : nullptr;
    ArgCheck a;
    a.writes(d_sin_lat, px, 4);
    a.writes(d_up, mul_sat(px, 2), 4);
    a.writes(d_lat, px, 4);
    a.writes(up_conf, px, 4);
    a.writes(lat_conf, px, 4);
    a.reads(d_up_raw, mul_sat(raw, 2), 2);
    a.reads(d_lat_raw, raw, 2);
    a.reads(d_up_logconf, raw, 2);
    a.reads(d_lat_logconf, raw, 2);
    if (!a.pass()) return -3;
    bool vec = ((size_t)H * W) % 8 == 0;
    for (const void* p : {d_up_raw, d_up_logconf, d_lat_raw, d_lat_logconf, (const void*)d_up, (const void*)up_conf, (const void*)d_lat,
                          (const void*)lat_conf, (const void*)d_sin_lat})
        vec = vec && is_aligned(p, 16);
    return launched(launch_pack_fields_typed(raw_dtype, d_up_raw, d_up_logconf, d_lat_raw, d_lat_logconf, B, H, W, vec, d_up, up_conf,
                                             d_lat, lat_conf, d_sin_lat, static_cast<hipStream_t>(stream)));
}

int gclm_pack_fields_backward(int raw_dtype, const void* d_up_raw, const void* d_up_logconf, const void* d_lat_raw,
                              const void* d_lat_logconf, int B, int H, int W, const float* d_g_up, const float* d_g_up_conf,
                              const float* d_g_lat, const float* d_g_lat_conf, void* d_d_up_raw, void* d_d_up_logconf,
                              void* d_d_lat_raw, void* d_d_lat_logconf, void* stream) {
    if (raw_dtype != GCLM_LOGITS_F32 && raw_dtype != GCLM_LOGITS_F16 && raw_dtype != GCLM_LOGITS_BF16) return -3;
    if (B < 0 || H <= 0 || W <= 0 || (!d_d_up_raw && !d_d_up_logconf && !d_d_lat_raw && !d_d_lat_logconf)) return -3;
    // a gradient asked for needs the gradient of its output and its raw plane; a group not asked for is not read
    struct Group { const void* raw; const float* g; void* d; int planes; };
    const Group groups[] = {{d_up_raw, d_g_up, d_d_up_raw, 2}, {d_up_logconf, d_g_up_conf, d_d_up_logconf, 1},
                            {d_lat_raw, d_g_lat, d_d_lat_raw, 1}, {d_lat_logconf, d_g_lat_conf, d_d_lat_logconf, 1}};
    for (const Group& g : groups)
        if (g.d && (!g.raw || !g.g)) return -3;
    const size_t esize = raw_dtype == GCLM_LOGITS_F32 ? 4 : 2, px = floats(B, H, W), raw = mul_sat(elements<char>(B, H, W), esize);
    ArgCheck a;
    for (const Group& g : groups) a.writes(g.d, mul_sat(raw, g.planes), esize);
    bool vec = ((size_t)H * W) % (esize == 4 ? 4 : 8) == 0;
    for (const Group& g : groups) {
        a.reads(g.raw, mul_sat(raw, g.planes), esize);      // (every plane given is held to the rules, read or not)
        a.reads(g.g, mul_sat(px, g.planes), 4);
        if (g.d) vec = vec && is_aligned(g.raw, 16) && is_aligned(g.g, 16) && is_aligned(g.d, 16);
    }
    if (!a.pass()) return -3;
    return launched(launch_pack_fields_backward(raw_dtype, d_up_raw, d_up_logconf, d_lat_raw, d_lat_logconf, B, H, W, vec, d_g_up,
                                                d_g_up_conf, d_g_lat, d_g_lat_conf, d_d_up_raw, d_d_up_logconf, d_d_lat_raw,
                                                d_d_lat_logconf, static_cast<hipStream_t>(stream)));
}

int gclm_pack_fields_bins(const void* d_up_logits, int up_bins, const void* d_lat_logits, int lat_bins, int logit_dtype,
                          const float* d_up_table, const float* d_lat_table, const float* d_up_logconf,
                          const float* d_lat_logconf, int B, int H, int W, float* d_up, float* d_up_conf, float* d_lat,
                          float* d_lat_conf, float* d_sin_lat, void* stream) {
    if (!d_up_logits || !d_lat_logits || !d_up_table || !d_lat_table || !d_up || !d_lat || B < 0 || H <= 0 || W <= 0) return -3;
    if (up_bins < 2 || up_bins > GCLM_MAX_BINS || lat_bins < 1 || lat_bins > GCLM_MAX_BINS) return -3;
    if (logit_dtype != GCLM_LOGITS_F32 && logit_dtype != GCLM_LOGITS_F16 && logit_dtype != GCLM_LOGITS_BF16) return -3;
    if ((d_up_logconf && !d_up_conf) || (d_lat_logconf && !d_lat_conf)) return -3;
    // Every output keeps off every other plane of the call, with one exception: a log-confidence that IS its output is
    // converted in place, lane by lane, and is not stated a second time as a range read.  A confidence output without its
    // log-confidence is not written and names no range.
    const size_t esize = logit_dtype == GCLM_LOGITS_F32 ? 4 : 2, px = floats(B, H, W);
    float* const up_conf = d_up_logconf ? d_up_conf : nullptr;
    float* const lat_conf = d_lat_logconf ? d_lat_conf : nullptr;
    const float* const up_lc = d_up_logconf == up_conf ? nullptr : d_up_logconf;
    const float* const lat_lc = d_lat_logconf == lat_conf ? nullptr : d_lat_logconf;
    ArgCheck a;
    a.writes(d_sin_lat, px, 4);
    a.writes(d_up, mul_sat(px, 2), 4);
    a.writes(d_lat, px, 4);
    a.writes(up_conf, px, 4);
    a.writes(lat_conf, px, 4);
    a.reads(d_up_logits, mul_sat(elements<char>(B, up_bins, H, W), esize), esize);
    a.reads(d_lat_logits, mul_sat(elements<char>(B, lat_bins, H, W), esize), esize);
    a.reads(d_up_table, floats(up_bins, 2), 4);
    a.reads(d_lat_table, floats(lat_bins), 4);
    a.reads(up_lc, px, 4);
    a.reads(lat_lc, px, 4);
    if (!a.pass()) return -3;
    bool vec = ((size_t)H * W) % (esize == 4 ? 4 : 8) == 0;
    for (const void* p : {d_up_logits, d_lat_logits, (const void*)d_up_logconf, (const void*)d_lat_logconf, (const void*)d_up,
                          (const void*)up_conf, (const void*)d_lat, (const void*)lat_conf, (const void*)d_sin_lat})
        vec = vec && is_aligned(p, 16);
    return launched(launch_pack_fields_bins(d_up_logits, up_bins, d_lat_logits, lat_bins, logit_dtype, d_up_table, d_lat_table,
                                            d_up_logconf, d_lat_logconf, B, H, W, vec, d_up, up_conf, d_lat, lat_conf, d_sin_lat,
                                            static_cast<hipStream_t>(stream)));
}

int gclm_undistort_image(int camera_model, const float* d_cam, int cam_batch, const float* d_src, int B, int C, int Hin, int Win,
                         int H, int W, float* d_dst, void* stream) {
    return undistort_image(camera_model, d_cam, cam_batch, d_src, B, C, Hin, Win, H, W, 0, d_dst, stream);
}

int gclm_undistort_image_u8(int camera_model, const float* d_cam, int cam_batch, const unsigned char* d_src, int B, int C, int Hin,
                            int Win, int H, int W, int interleaved, unsigned char* d_dst, void* stream) {
    return undistort_image(camera_model, d_cam, cam_batch, d_src, B, C, Hin, Win, H, W, interleaved, d_dst, stream);
}

int gclm_reproject_image(int src_model, const float* d_src_cam, int dst_model, const float* d_dst_cam, int cam_batch,
                         const float* d_rot, int rot_batch, const float* d_src, int B, int C, int Hin, int Win, int Hs, int Ws,
                         int H, int W, float* d_dst, unsigned char* d_valid, void* stream) {
    return reproject_image(src_model, d_src_cam, dst_model, d_dst_cam, cam_batch, d_rot, rot_batch, d_src, B, C, Hin, Win, Hs, Ws,
                           H, W, 0, d_dst, d_valid, stream);
}

int gclm_reproject_image_u8(int src_model, const float* d_src_cam, int dst_model, const float* d_dst_cam, int cam_batch,
                            const float* d_rot, int rot_batch, const unsigned char* d_src, int B, int C, int Hin, int Win, int Hs,
                            int Ws, int H, int W, int interleaved, unsigned char* d_dst, unsigned char* d_valid, void* stream) {
    return reproject_image(src_model, d_src_cam, dst_model, d_dst_cam, cam_batch, d_rot, rot_batch, d_src, B, C, Hin, Win, Hs, Ws,
                           H, W, interleaved, d_dst, d_valid, stream);
}

int gclm_draw_fields(int camera_model, const float* d_cam, const float* d_grav, int cal_batch, const float* d_src, int B, int C,
                     int H, int W, const float* d_conf, const unsigned char* d_palette, const unsigned char* d_heat_palette,
                     const gclm_overlay_style* style, float* d_dst, void* stream) {
    return draw_fields(camera_model, d_cam, d_grav, cal_batch, d_src, B, C, H, W, 0, d_conf, d_palette, d_heat_palette, style, d_dst,
                       stream);
}

int gclm_draw_fields_u8(int camera_model, const float* d_cam, const float* d_grav, int cal_batch, const unsigned char* d_src, int B,
                        int C, int H, int W, int interleaved, const float* d_conf, const unsigned char* d_palette,
                        const unsigned char* d_heat_palette, const gclm_overlay_style* style, unsigned char* d_dst, void* stream) {
    return draw_fields(camera_model, d_cam, d_grav, cal_batch, d_src, B, C, H, W, interleaved, d_conf, d_palette, d_heat_palette,
                       style, d_dst, stream);
}

int gclm_perspective_fields(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, int normalize_up,
                            float* d_up, float* d_lat, void* stream) {
    if (!d_cam || !d_grav || (!d_up && !d_lat) || B < 1 || B > kMaxCallImages || H < 1 || W < 1) return -3;
    if (!known_model(camera_model) || (normalize_up != 0 && normalize_up != 1) || !tile_grid_fits(H, W)) return -3;
    if (!is_aligned(d_up, 8) || !is_aligned(d_lat, 4)) return -3;      // (before any range arithmetic, as ever)
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_up, mul_sat(px, 2));
    a.writes(d_lat, px);
    a.reads(d_cam, floats(B, 8));
    a.reads(d_grav, floats(B, 3));
    if (!a.pass()) return -3;
    return launched(launch_perspective_fields(camera_model, d_cam, d_grav, B, H, W, normalize_up, d_up, d_lat,
                                              static_cast<hipStream_t>(stream)));
}

size_t gclm_field_errors_workspace(int B, int H, int W, int n_thresholds) {
    return field_errors_workspace(B, H, W, n_thresholds);
}

int gclm_field_errors(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const float* d_up,
                      const float* d_lat, const float* d_up_conf, const float* d_lat_conf, int n_thresholds,
                      const float* thresholds_deg, void* d_workspace, size_t workspace_bytes, float* d_stats, float* d_up_err,
                      float* d_lat_err, void* stream) {
    if (!d_cam || !d_grav || !d_stats || !d_workspace || (!d_up && !d_lat)) return -3;
    if ((!d_up && (d_up_conf || d_up_err)) || (!d_lat && (d_lat_conf || d_lat_err)) || !known_model(camera_model)) return -3;
    const size_t ws_bytes = field_errors_workspace(B, H, W, n_thresholds);       // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes || (n_thresholds > 0 && !thresholds_deg)) return -3;
    for (int k = 0; k < n_thresholds; ++k)
        if (!(fabsf(thresholds_deg[k]) <= FLT_MAX)) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_stats, floats(B, 2, 2 + n_thresholds), 4);
    a.writes(d_workspace, ws_bytes, 4);
    a.writes(d_up_err, px, 4);
    a.writes(d_lat_err, px, 4);
    a.reads(d_cam, floats(B, 8), 4);
    a.reads(d_grav, floats(B, 3), 4);
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_up_conf, px, 4);
    a.reads(d_lat_conf, px, 4);
    if (!a.pass()) return -3;
    return launched(launch_field_errors(camera_model, d_cam, d_grav, B, H, W, d_up, d_lat, d_up_conf, d_lat_conf, n_thresholds,
                                        thresholds_deg, d_workspace, d_stats, d_up_err, d_lat_err, static_cast<hipStream_t>(stream)));
}

size_t gclm_field_loss_workspace(int B, int H, int W) { return field_loss_workspace(B, H, W); }

int gclm_field_loss(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const float* d_up,
                    const float* d_lat, const float* d_up_conf, const float* d_lat_conf, int up_loss, int lat_loss,
                    void* d_workspace, size_t workspace_bytes, float* d_out, void* stream) {
    if (!d_out || !d_workspace) return -3;
    if (!field_loss_plain_ok(camera_model, d_cam, d_grav, d_up, d_lat, d_up_conf, d_lat_conf, up_loss, lat_loss)) return -3;
    const size_t ws_bytes = field_loss_workspace(B, H, W);                       // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_out, floats(B, 4), 4);
    a.writes(d_workspace, ws_bytes, 4);
    a.reads(d_cam, floats(B, 8), 4);
    a.reads(d_grav, floats(B, 3), 4);
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_up_conf, px, 4);
    a.reads(d_lat_conf, px, 4);
    if (!a.pass()) return -3;
    return launched(launch_field_loss(camera_model, d_cam, d_grav, B, H, W, d_up, d_lat, d_up_conf, d_lat_conf, up_loss, lat_loss,
                                      d_workspace, d_out, static_cast<hipStream_t>(stream)));
}

int gclm_field_loss_grad(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const float* d_up,
                         const float* d_lat, const float* d_up_conf, const float* d_lat_conf, int up_loss, int lat_loss,
                         const float* d_scale, float* d_grad_up, float* d_grad_lat, void* stream) {
    if (!d_scale || (d_up != nullptr) != (d_grad_up != nullptr) || (d_lat != nullptr) != (d_grad_lat != nullptr)) return -3;
    if (!field_loss_plain_ok(camera_model, d_cam, d_grav, d_up, d_lat, d_up_conf, d_lat_conf, up_loss, lat_loss)) return -3;
    if (field_loss_workspace(B, H, W) == 0) return -3;                           // (the sizes the forward refuses)
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_grad_up, mul_sat(px, 2), 4);
    a.writes(d_grad_lat, px, 4);
    a.reads(d_cam, floats(B, 8), 4);
    a.reads(d_grav, floats(B, 3), 4);
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_up_conf, px, 4);
    a.reads(d_lat_conf, px, 4);
    a.reads(d_scale, floats(B, 2), 4);
    if (!a.pass()) return -3;
    return launched(launch_field_loss_grad(camera_model, d_cam, d_grav, B, H, W, d_up, d_lat, d_up_conf, d_lat_conf, up_loss, lat_loss,
                                           d_scale, d_grad_up, d_grad_lat, static_cast<hipStream_t>(stream)));
}

size_t gclm_bin_loss_workspace(int B, int H, int W) { return bin_loss_workspace(B, H, W); }

int gclm_bin_loss(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const void* d_up_logits, int up_bins,
                  const void* d_lat_logits, int lat_bins, int logit_dtype, const float* d_up_conf, const float* d_lat_conf,
                  void* d_workspace, size_t workspace_bytes, float* d_out, float* d_lse, int16_t* d_bins, void* stream) {
    if (!d_cam || !d_grav || !d_workspace || !d_out || !d_lse || !d_bins || !known_model(camera_model)) return -3;
    if (!bin_loss_plain_ok(d_up_logits, up_bins, d_lat_logits, lat_bins, logit_dtype, d_up_conf, d_lat_conf, B, H, W)) return -3;
    if (B == 0) return 0;
    const size_t ws_bytes = bin_loss_workspace(B, H, W);                         // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes) return -3;
    const size_t esize = logit_dtype == GCLM_LOGITS_F32 ? 4 : 2, px = floats(B, H, W);
    ArgCheck a;
    a.writes(d_out, floats(B, 6), 4);
    a.writes(d_lse, mul_sat(px, 2), 4);
    a.writes(d_bins, elements<int16_t>(B, 2, H, W), 2);
    a.writes(d_workspace, ws_bytes, 4);
    a.reads(d_cam, floats(B, 8), 4);
    a.reads(d_grav, floats(B, 3), 4);
    a.reads(d_up_logits, mul_sat(elements<char>(B, up_bins, H, W), esize), esize);
    a.reads(d_lat_logits, mul_sat(elements<char>(B, lat_bins, H, W), esize), esize);
    a.reads(d_up_conf, px, 4);
    a.reads(d_lat_conf, px, 4);
    if (!a.pass()) return -3;
    return launched(launch_bin_loss(camera_model, d_cam, d_grav, B, H, W, d_up_logits, up_bins, d_lat_logits, lat_bins, logit_dtype,
                                    d_up_conf, d_lat_conf, d_workspace, d_out, d_lse, d_bins, static_cast<hipStream_t>(stream)));
}

int gclm_bin_loss_grad(const void* d_up_logits, int up_bins, const void* d_lat_logits, int lat_bins, int logit_dtype,
                       const float* d_up_conf, const float* d_lat_conf, int B, int H, int W, const float* d_lse, const int16_t* d_bins,
                       const float* d_scale, void* d_grad_up, void* d_grad_lat, void* stream) {
    if (!d_lse || !d_bins || !d_scale || (!d_grad_up && !d_grad_lat) || (d_grad_up && !d_up_logits) || (d_grad_lat && !d_lat_logits)) return -3;
    if (!bin_loss_plain_ok(d_up_logits, up_bins, d_lat_logits, lat_bins, logit_dtype, d_up_conf, d_lat_conf, B, H, W)) return -3;
    if (B == 0) return 0;
    if (bin_loss_workspace(B, H, W) == 0) return -3;                             // (the sizes the forward refuses)
    const size_t esize = logit_dtype == GCLM_LOGITS_F32 ? 4 : 2, px = floats(B, H, W);
    const size_t up_bytes = mul_sat(elements<char>(B, up_bins, H, W), esize), lat_bytes = mul_sat(elements<char>(B, lat_bins, H, W), esize);
    ArgCheck a;
    a.writes(d_grad_up, up_bytes, esize);
    a.writes(d_grad_lat, lat_bytes, esize);
    a.reads(d_up_logits, up_bytes, esize);
    a.reads(d_lat_logits, lat_bytes, esize);
    a.reads(d_up_conf, px, 4);
    a.reads(d_lat_conf, px, 4);
    a.reads(d_lse, mul_sat(px, 2), 4);
    a.reads(d_bins, elements<int16_t>(B, 2, H, W), 2);
    a.reads(d_scale, floats(B, 2), 4);
    if (!a.pass()) return -3;
    return launched(launch_bin_loss_grad(B, H, W, d_up_logits, up_bins, d_lat_logits, lat_bins, logit_dtype, d_up_conf, d_lat_conf, d_lse,
                                         d_bins, d_scale, d_grad_up, d_grad_lat, static_cast<hipStream_t>(stream)));
}

size_t gclm_field_param_grad_workspace(int B, int H, int W) { return field_param_grad_workspace(B, H, W); }

int gclm_field_loss_param_grad(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, const float* d_up,
                               const float* d_lat, const float* d_up_conf, const float* d_lat_conf, int up_loss, int lat_loss,
                               const float* d_scale, void* d_workspace, size_t workspace_bytes, float* d_grad_cam,
                               float* d_grad_grav, void* stream) {
    if (!d_scale || !d_workspace || (!d_grad_cam && !d_grad_grav)) return -3;
    if (!field_loss_plain_ok(camera_model, d_cam, d_grav, d_up, d_lat, d_up_conf, d_lat_conf, up_loss, lat_loss)) return -3;
    const size_t ws_bytes = field_param_grad_workspace(B, H, W);                 // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_grad_cam, floats(B, 8), 4);
    a.writes(d_grad_grav, floats(B, 3), 4);
    a.writes(d_workspace, ws_bytes, 8);
    a.reads(d_cam, floats(B, 8), 4);
    a.reads(d_grav, floats(B, 3), 4);
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_up_conf, px, 4);
    a.reads(d_lat_conf, px, 4);
    a.reads(d_scale, floats(B, 2), 4);
    if (!a.pass()) return -3;
    return launched(launch_field_loss_param_grad(camera_model, d_cam, d_grav, B, H, W, d_up, d_lat, d_up_conf, d_lat_conf, up_loss,
                                                 lat_loss, d_scale, d_workspace, d_grad_cam, d_grad_grav,
                                                 static_cast<hipStream_t>(stream)));
}

int gclm_perspective_fields_backward(int camera_model, const float* d_cam, const float* d_grav, int B, int H, int W, int normalize_up,
                                     const float* d_grad_up, const float* d_grad_lat, void* d_workspace, size_t workspace_bytes,
                                     float* d_grad_cam, float* d_grad_grav, void* stream) {
    if (!d_cam || !d_grav || (!d_grad_up && !d_grad_lat) || !d_workspace || (!d_grad_cam && !d_grad_grav)) return -3;
    if (!known_model(camera_model) || (normalize_up != 0 && normalize_up != 1)) return -3;
    const size_t ws_bytes = field_param_grad_workspace(B, H, W);                 // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_grad_cam, floats(B, 8), 4);
    a.writes(d_grad_grav, floats(B, 3), 4);
    a.writes(d_workspace, ws_bytes, 8);
    a.reads(d_cam, floats(B, 8), 4);
    a.reads(d_grav, floats(B, 3), 4);
    a.reads(d_grad_up, mul_sat(px, 2), 8);                                       // (pairs, as gclm_perspective_fields writes them)
    a.reads(d_grad_lat, px, 4);
    if (!a.pass()) return -3;
    return launched(launch_perspective_fields_backward(camera_model, d_cam, d_grav, B, H, W, normalize_up, d_grad_up, d_grad_lat,
                                                       d_workspace, d_grad_cam, d_grad_grav, static_cast<hipStream_t>(stream)));
}

size_t gclm_lm_backward_workspace(int B, int H, int W) { return lm_backward_workspace(B, H, W); }

int gclm_lm_backward(int camera_model, const float* d_up, const float* d_lat, const float* d_up_conf, const float* d_lat_conf,
                     int B, int H, int W, const float* d_record, int num_steps, int early_stop, const float* d_info,
                     float up_scale, float lat_scale, int estimate_gravity, int estimate_focal, int estimate_dist,
                     const float* d_grad_cam, const float* d_grad_grav, float* d_grad_up, float* d_grad_lat,
                     float* d_grad_up_conf, float* d_grad_lat_conf, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (camera_model != GCLM_PINHOLE && camera_model != GCLM_SIMPLE_RADIAL) return -3;
    if (!d_lat || !d_record || !d_grad_cam || !d_grad_grav || !d_workspace || (early_stop && !d_info)) return -3;
    if (num_steps < 1 || num_steps > GCLM_MAX_STEPS || !(up_scale > 0.f) || !(lat_scale > 0.f)) return -3;
    // a gradient plane only for an input that is there (the up confidence counts only beside the up field)
    if ((d_grad_up && !d_up) || (d_grad_up_conf && !(d_up && d_up_conf)) || (d_grad_lat_conf && !d_lat_conf)) return -3;
    const size_t ws_bytes = lm_backward_workspace(B, H, W);                      // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_grad_up, mul_sat(px, 2), 4);
    a.writes(d_grad_lat, px, 4);
    a.writes(d_grad_up_conf, px, 4);
    a.writes(d_grad_lat_conf, px, 4);
    a.writes(d_workspace, ws_bytes, 8);
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_up_conf, px, 4);
    a.reads(d_lat_conf, px, 4);
    a.reads(d_record, floats(B, num_steps, GCLM_LM_RECORD_STRIDE), 4);
    a.reads(d_info, floats(B, GCLM_INFO_STRIDE), 4);
    a.reads(d_grad_cam, floats(B, 8), 4);
    a.reads(d_grad_grav, floats(B, 3), 4);
    if (!a.pass()) return -3;
    return launched(launch_lm_backward(camera_model, d_up, d_lat, d_up_conf, d_lat_conf, B, H, W, d_record, num_steps, early_stop,
                                       d_info, up_scale, lat_scale, estimate_gravity, estimate_focal, estimate_dist, d_grad_cam,
                                       d_grad_grav, d_grad_up, d_grad_lat, d_grad_up_conf, d_grad_lat_conf, d_workspace,
                                       static_cast<hipStream_t>(stream)));
}

size_t gclm_hypothesis_scores_workspace(int B, int N, int H, int W) { return hypothesis_scores_workspace(B, N, H, W); }

int gclm_hypothesis_scores(int camera_model, const float* d_cam, const float* d_grav, int B, int N, int H, int W,
                           const float* d_up, const float* d_lat, const float* d_up_conf, const float* d_lat_conf,
                           const float* d_mask, float up_threshold_deg, float lat_threshold_deg, float up_weight, float lat_weight,
                           void* d_workspace, size_t workspace_bytes, float* d_scores, int* d_best, void* stream) {
    if (!d_cam || !d_grav || !d_scores || !d_workspace || (!d_up && !d_lat)) return -3;
    if ((!d_up && d_up_conf) || (!d_lat && d_lat_conf) || !known_model(camera_model)) return -3;
    const size_t ws_bytes = hypothesis_scores_workspace(B, N, H, W);             // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes) return -3;
    for (const float v : {up_threshold_deg, lat_threshold_deg, up_weight, lat_weight})
        if (!(fabsf(v) <= FLT_MAX)) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_scores, floats(B, N, 3), 4);
    a.writes(d_best, mul_sat((size_t)B, sizeof(int)), 4);
    a.writes(d_workspace, ws_bytes, 4);
    a.reads(d_cam, floats(B, N, 8), 4);
    a.reads(d_grav, floats(B, N, 3), 4);
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_up_conf, px, 4);
    a.reads(d_lat_conf, px, 4);
    a.reads(d_mask, px, 4);
    if (!a.pass()) return -3;
    return launched(launch_hypothesis_scores(camera_model, d_cam, d_grav, B, N, H, W, d_up, d_lat, d_up_conf, d_lat_conf, d_mask,
                                             up_threshold_deg, lat_threshold_deg, up_weight, lat_weight, d_workspace, d_scores,
                                             d_best, static_cast<hipStream_t>(stream)));
}

int gclm_default_param_opt_config(gclm_param_opt_config* config) {
    if (!config) return -3;
    // PerspectiveParamOpt.default_conf, perspective_opt.py:24-36, and torch's ReduceLROnPlateau defaults
    *config = gclm_param_opt_config{(int32_t)sizeof(gclm_param_opt_config), 1000, 3, 1, 3, 0, 16, 0, 0.01, 1e-7, 1e-9, 0.5, 0.1, 1e-4, 0.0, 1e-8};
    return 0;
}

size_t gclm_param_opt_workspace(int B, int H, int W) { return param_opt_workspace(B, H, W); }

int gclm_param_opt_cost(const float* d_up, const float* d_lat, const float* d_rpv, int B, int H, int W, void* d_workspace,
                        size_t workspace_bytes, float* d_out, void* stream) {
    if (!d_up || !d_lat || !d_rpv || !d_workspace || !d_out) return -3;
    const size_t ws_bytes = param_opt_workspace(B, H, W);                        // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_out, floats(B, 8), 4);
    a.writes(d_workspace, ws_bytes, 16);
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_rpv, floats(B, 3), 4);
    if (!a.pass()) return -3;
    return launched(launch_param_opt_cost(d_up, d_lat, d_rpv, B, H, W, d_workspace, d_out, static_cast<hipStream_t>(stream)));
}

int gclm_param_opt_step(void* d_state, const float* d_cost, int B, const gclm_param_opt_config* config, void* stream) {
    if (!d_state || !d_cost || !config || B < 1 || B > kMaxCallImages || !param_opt_config_ok(*config)) return -3;
    ArgCheck a;
    a.writes(d_state, floats(B, GCLM_PARAM_OPT_STATE_WORDS), 8);
    a.reads(d_cost, floats(B, 8), 4);
    if (!a.pass()) return -3;
    return launched(launch_param_opt_step(d_state, d_cost, B, *config, static_cast<hipStream_t>(stream)));
}

int gclm_param_opt(const float* d_up, const float* d_lat, const float* d_init_rpv, int B, int H, int W,
                   const gclm_param_opt_config* config, void* d_workspace, size_t workspace_bytes, float* d_rpv, float* d_info,
                   void* stream) {
    if (!d_up || !d_lat || !config || !d_workspace || !d_rpv || !d_info || !param_opt_config_ok(*config)) return -3;
    const size_t ws_bytes = param_opt_workspace(B, H, W);                        // 0: sizes out of range
    if (ws_bytes == 0 || workspace_bytes < ws_bytes) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W);
    a.writes(d_rpv, floats(B, 3), 4);
    a.writes(d_info, floats(B, GCLM_PARAM_OPT_INFO_WORDS), 4);
    a.writes(d_workspace, ws_bytes, 16);
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_init_rpv, floats(B, 3), 4);
    if (!a.pass()) return -3;
    return launched(launch_param_opt(d_up, d_lat, d_init_rpv, B, H, W, *config, d_workspace, d_rpv, d_info,
                                     static_cast<hipStream_t>(stream)));
}

int gclm_rpf_hypotheses(const float* d_up, const float* d_lat, const float* d_prior_focal, const int32_t* d_samples, uint64_t seed,
                        int64_t first_index, int B, int N, int H, int W, float* d_cam, float* d_grav, int32_t* d_samples_out,
                        void* stream) {
    if (!d_up || !d_cam || !d_grav || (!d_lat && !d_prior_focal)) return -3;
    if (B < 1 || B > kMaxCallImages || N < 1 || N > GCLM_RPF_MAX_SAMPLES || H < 1 || W < 1 || (int64_t)H * W > INT32_MAX) return -3;
    ArgCheck a;
    const size_t px = floats(B, H, W), rows = mul_sat((size_t)N, d_prior_focal ? 1 : 2);
    a.writes(d_cam, floats(B, rows, 8), 4);
    a.writes(d_grav, floats(B, rows, 3), 4);
    a.writes(d_samples_out, floats(B, N, 6), 4);          // (int32: as wide as a float)
    a.reads(d_up, mul_sat(px, 2), 4);
    a.reads(d_lat, px, 4);
    a.reads(d_prior_focal, floats(B), 4);
    a.reads(d_samples, floats(B, N, 6), 4);
    if (!a.pass()) return -3;
    return launched(launch_rpf_hypotheses(d_up, d_lat, d_prior_focal, d_samples, seed, first_index, B, N, H, W, d_cam, d_grav,
                                          d_samples_out, static_cast<hipStream_t>(stream)));
}

int gclm_render_from_pano(int camera_model, const float* d_cam, int cam_batch, const float* d_rot, const float* const* srcs,
                          const int* src_hw, int n, int C, int H, int W, float* d_dst, void* stream) {
    if (!d_cam || !d_rot || !srcs || !src_hw || !d_dst || n < 1 || n > kMaxCallImages || C < 1 || H < 2 || W < 2) return -3;
    if ((cam_batch != 1 && cam_batch != n) || !known_model(camera_model) || (int64_t)H * W > INT32_MAX) return -3;
    ArgCheck a;
    a.writes(d_dst, floats(n, C, H, W));
    a.reads(d_cam, floats(cam_batch, 8));
    a.reads(d_rot, floats(n, 9));
    if (!a.pass()) return -3;
    for (int i = 0; i < n; ++i) {             // (no table entry is read behind the first bad one)
        const int Hs = src_hw[2 * i], Ws = src_hw[2 * i + 1];
        if (!srcs[i] || Hs < 2 || Ws < 2) return -3;
        a.reads(srcs[i], floats(C, Hs, Ws));
        if (!a.pass()) return -3;
    }
    return launched(launch_render_from_pano(camera_model, d_cam, cam_batch, d_rot, srcs, src_hw, n, C, H, W, d_dst,
                                            static_cast<hipStream_t>(stream)));
}

int gclm_read_probe(const float* const* d_planes, int n_planes, size_t n_floats, void* stream) {
    if (!d_planes || n_planes < 1 || n_planes > 8 || n_floats % 4 != 0) return -3;
    for (int k = 0; k < n_planes; ++k)
        if (!d_planes[k] || !is_aligned(d_planes[k], 16)) return -3;
    return launched(launch_read_probe(d_planes, n_planes, n_floats, static_cast<hipStream_t>(stream)));
}

int gclm_synth_fields_grouped(int camera_model, uint64_t seed, int64_t first_index, int B, int H, int W,
                              float noise_sigma, int group_size, int run, int run_stride, float* d_up,
                              float* d_lat, float* d_up_conf, float* d_lat_conf, float* d_gt_cam,
                              float* d_gt_grav, void* stream) {
    if (!d_up || !d_lat || B < 0 || H <= 0 || W <= 0 || group_size < 0 || run < 0) return -3;
    if (!known_model(camera_model)) return -2;
    return launched(launch_synth(camera_model, seed, first_index, B, H, W, noise_sigma, group_size, run, run_stride,
                                 d_up, d_lat, d_up_conf, d_lat_conf, d_gt_cam, d_gt_grav, static_cast<hipStream_t>(stream)));
}

int gclm_synth_fields(int camera_model, uint64_t seed, int64_t first_index, int B, int H, int W,
                      float noise_sigma, float* d_up, float* d_lat, float* d_up_conf, float* d_lat_conf,
                      float* d_gt_cam, float* d_gt_grav, void* stream) {
    return gclm_synth_fields_grouped(camera_model, seed, first_index, B, H, W, noise_sigma, 1, 0, 0, d_up, d_lat,
                                     d_up_conf, d_lat_conf, d_gt_cam, d_gt_grav, stream);
}

}  // extern "C"
