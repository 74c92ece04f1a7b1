// gclm_fields.hip -- the steps before and after the path: the CNN-head epilogue that packs the planes a sweep reads
// (gclm_pack_fields; gclm_pack_fields_typed for 16-bit raws; gclm_pack_fields_bins for classification heads), that epilogue's
// backward (gclm_pack_fields_backward) and the bilinear upsampler of GeoCalib._post_process (gclm_upsample_fields).  Per-pixel
// streaming kernels; nothing here knows about the solve.
#include "gclm_device.h"
#include "gclm_logits.h"

namespace gclm {

namespace {

// (the typed planes -- bins_elem, bins_vec, kBinsUnroll, bins_widen, bins_load, pack_narrow -- are gclm_logits.h's, shared with
// gclm_bin_loss.hip; bins_u4 / bins_f4 too)
template <int VEC>
__device__ __forceinline__ void bins_load_f32(const float* p, size_t i, float (&v)[VEC]) {
    if constexpr (VEC == 1) v[0] = p[i];
    else {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
            const bins_f4 t = __builtin_nontemporal_load(reinterpret_cast<const bins_f4*>(p) + i * (VEC / 4) + q);
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    }
}
template <int VEC>
__device__ __forceinline__ void bins_store_f32(float* p, size_t i, const float (&v)[VEC]) {
    if constexpr (VEC == 1) p[i] = v[0];
    else {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q)
            __builtin_nontemporal_store(bins_f4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]},
                                        reinterpret_cast<bins_f4*>(p) + i * (VEC / 4) + q);
    }
}

// ---------------------------------------------------------------- CNN-head epilogue (the step before the path)
// UpDecoder / LatitudeDecoder epilogues (geocalib.py:57,73-75) fused into ONE pass that writes the five
// planes the sweep reads: up = normalize(raw, dim=1), latitude = asin(clamp(tanh(raw), +-(1-1e-5))),
// confidences = sigmoid(log-confidence).  Eager PyTorch runs 8 elementwise kernels and ~18 plane passes.
// slat (gclm_pack_fields_ex; NULL: not written): a sixth plane, sin of the latitude just written, by the sweep's own
// polynomial (dev::sin_halfpi) -- the floats a sweep would compute from `lat`, so a solve that reads this plane in place of
// the radians gives the same bits.  The packed latitude lies within +-asin(1 - 1e-5) < pi/2: the range fold the sweep keeps
// for a caller's own radians (gclm_pass.hip: row_slat) never fires on it and is not needed here.
// DT (gclm_pack_fields_typed): the raw planes' type.  float32 is the kernel as it always was; 16-bit raws widen exactly on
// load, eight per lane on the vector walk (one 16-byte load per plane, two 16-byte stores per float32 output), and the
// arithmetic below is the same float32 expressions -- the bits of the float32 kernel on the widened planes.
template <int VEC, int DT = GCLM_LOGITS_F32>
__global__ void pack_fields_kernel(const bins_elem<DT>* __restrict__ up_raw, const bins_elem<DT>* __restrict__ up_lc,
                                   const bins_elem<DT>* __restrict__ lat_raw, const bins_elem<DT>* __restrict__ lat_lc, int B,
                                   size_t N, float* __restrict__ up, float* __restrict__ upc,
                                   float* __restrict__ lat, float* __restrict__ latc, float* __restrict__ slat) {
    const size_t units = N / VEC;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const bins_elem<DT>* ux = up_raw + (size_t)b * 2 * N;
        const bins_elem<DT>* uy = ux + N;
        float* ox = up + (size_t)b * 2 * N;
        float* oy = ox + N;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += (size_t)gridDim.x * blockDim.x) {
            float vx[VEC], vy[VEC], vl[VEC], c1[VEC], c2[VEC], sl[VEC];
            if constexpr (DT != GCLM_LOGITS_F32) {
                bins_load<DT, VEC>(ux, i, vx); bins_load<DT, VEC>(uy, i, vy); bins_load<DT, VEC>(lat_raw + (size_t)b * N, i, vl);
                if (up_lc) bins_load<DT, VEC>(up_lc + (size_t)b * N, i, c1);
                if (lat_lc) bins_load<DT, VEC>(lat_lc + (size_t)b * N, i, c2);
            } else if constexpr (VEC == 4) {
                // every byte is read once and written once: non-temporal both ways (+4 ... 8 % over plain float4 accesses,
                // profiles/archive/r05_pack_bench.log)
                typedef float pk4 __attribute__((ext_vector_type(4)));
                auto ld4 = [](const float* p, size_t j) { return __builtin_nontemporal_load(reinterpret_cast<const pk4*>(p) + j); };
                const pk4 a = ld4(ux, i), bq = ld4(uy, i), l = ld4(lat_raw + (size_t)b * N, i);
                vx[0] = a.x; vx[1] = a.y; vx[2] = a.z; vx[3] = a.w;
                vy[0] = bq.x; vy[1] = bq.y; vy[2] = bq.z; vy[3] = bq.w;
                vl[0] = l.x; vl[1] = l.y; vl[2] = l.z; vl[3] = l.w;
                if (up_lc) { const pk4 t = ld4(up_lc + (size_t)b * N, i); c1[0] = t.x; c1[1] = t.y; c1[2] = t.z; c1[3] = t.w; }
                if (lat_lc) { const pk4 t = ld4(lat_lc + (size_t)b * N, i); c2[0] = t.x; c2[1] = t.y; c2[2] = t.z; c2[3] = t.w; }
            } else {
                vx[0] = ux[i]; vy[0] = uy[i]; vl[0] = lat_raw[(size_t)b * N + i];
                if (up_lc) c1[0] = up_lc[(size_t)b * N + i];
                if (lat_lc) c2[0] = lat_lc[(size_t)b * N + i];
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float n = fmaxf(sqrtf(vx[k] * vx[k] + vy[k] * vy[k]), 1e-12f);     // F.normalize eps
                vx[k] /= n; vy[k] /= n;
                vl[k] = asinf(fminf(fmaxf(tanhf(vl[k]), -1.0f + 1e-5f), 1.0f - 1e-5f));
                if (slat) sl[k] = dev::sin_halfpi(vl[k]);
                if (up_lc) c1[k] = 1.0f / (1.0f + expf(-c1[k]));
                if (lat_lc) c2[k] = 1.0f / (1.0f + expf(-c2[k]));
            }
            if constexpr (VEC == 8) {
                const size_t j = (size_t)b * (N / VEC) + i;
                bins_store_f32<VEC>(ox, i, vx); bins_store_f32<VEC>(oy, i, vy); bins_store_f32<VEC>(lat, j, vl);
                if (up_lc) bins_store_f32<VEC>(upc, j, c1);
                if (lat_lc) bins_store_f32<VEC>(latc, j, c2);
                if (slat) bins_store_f32<VEC>(slat, j, sl);
            } else if constexpr (VEC == 4) {
                typedef float pk4 __attribute__((ext_vector_type(4)));
                auto st4 = [](float* p, size_t j, const float (&v)[VEC]) {
                    __builtin_nontemporal_store(pk4{v[0], v[1], v[2], v[3]}, reinterpret_cast<pk4*>(p) + j);
                };
                st4(ox, i, vx); st4(oy, i, vy); st4(lat + (size_t)b * N, i, vl);
                if (up_lc) st4(upc + (size_t)b * N, i, c1);
                if (lat_lc) st4(latc + (size_t)b * N, i, c2);
                if (slat) st4(slat + (size_t)b * N, i, sl);
            } else {
                ox[i] = vx[0]; oy[i] = vy[0]; lat[(size_t)b * N + i] = vl[0];
                if (up_lc) upc[(size_t)b * N + i] = c1[0];
                if (lat_lc) latc[(size_t)b * N + i] = c2[0];
                if (slat) slat[(size_t)b * N + i] = sl[0];
            }
        }
    }
}

// ---------------------------------------------------------------- the epilogue's backward (gclm_pack_fields_backward)
// The gradients of the four outputs above, g_*, taken back to the raw planes in ONE pass that reads the raws again and
// recomputes in float32 what it needs of the forward: no forward output is read, none has to be kept.  d_* are written in
// the raws' type, rounded to nearest even.  A group (up, latitude, either confidence) runs where its d_* is given -- wave-
// uniform branches, as the forward's; the entry has checked that such a group has its raw plane and its g_*.
//   up          n = |r|.  n >= 1e-12: with u = r / n and u' = (-u.y, u.x), d_r = u' (u' . g) / n -- in two dimensions this IS
//               g - u (u . g), without its cancellation where g is nearly parallel to u, and d_r . r = 0 to the rounding
//               of two products.  n < 1e-12 (the clamped branch of F.normalize): d_r = g / 1e-12.
//   latitude    asin(tanh x) has the derivative sech x = 2 e / (1 + e^2), e = exp(-|x|) (no cancellation; sqrt(1 - t^2) has
//               lost three digits at |x| = 6); exactly 0 where the forward's tanhf(x) left [-1 + 1e-5, 1 - 1e-5] -- the same
//               comparison on the same float, so forward and backward agree on every pixel about what was clamped.
//   confidence  s (1 - s) = e / (1 + e)^2, e = exp(-|x|): finite and >= 0 for every finite x.
// A NaN raw makes e (or n) NaN and with it the gradients of its own group only.
// The raws and the incoming gradients are read once: non-temporal loads.  The raw gradients are read by autograd's next
// kernel, so their stores were decided by a measurement with such a reader behind the pass: plain -- non-temporal
// stores win 6 % at B = 1024 and lose as much at B = 64, a training batch (GCLM_PACK_BWD_NT_STORES builds that variant).
template <int DT, int VEC>
__device__ __forceinline__ void pack_store_grad(bins_elem<DT>* p, size_t i, const float (&v)[VEC]) {
    if constexpr (VEC == 1) p[i] = pack_narrow<DT>(v[0]);
    else {
        bins_u4 q;
        if constexpr (DT == GCLM_LOGITS_F32) {
            q = bins_u4{__builtin_bit_cast(uint32_t, v[0]), __builtin_bit_cast(uint32_t, v[1]), __builtin_bit_cast(uint32_t, v[2]),
                        __builtin_bit_cast(uint32_t, v[3])};
        } else {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = (uint32_t)pack_narrow<DT>(v[2 * k]) | ((uint32_t)pack_narrow<DT>(v[2 * k + 1]) << 16);
            q = bins_u4{w[0], w[1], w[2], w[3]};
        }
#ifdef GCLM_PACK_BWD_NT_STORES
        __builtin_nontemporal_store(q, reinterpret_cast<bins_u4*>(p) + i);
#else
        reinterpret_cast<bins_u4*>(p)[i] = q;
#endif
    }
}
template <int DT, int VEC>
__global__ __launch_bounds__(256) void pack_fields_backward_kernel(
    const bins_elem<DT>* __restrict__ up_raw, const bins_elem<DT>* __restrict__ up_lc, const bins_elem<DT>* __restrict__ lat_raw,
    const bins_elem<DT>* __restrict__ lat_lc, int B, size_t N, const float* __restrict__ g_up, const float* __restrict__ g_upc,
    const float* __restrict__ g_lat, const float* __restrict__ g_latc, bins_elem<DT>* __restrict__ d_up,
    bins_elem<DT>* __restrict__ d_upc, bins_elem<DT>* __restrict__ d_lat, bins_elem<DT>* __restrict__ d_latc) {
    const size_t units = N / VEC;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const size_t up0 = (size_t)b * 2 * units, px0 = (size_t)b * units;      // in units: N is a multiple of VEC
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += (size_t)gridDim.x * blockDim.x) {
            float vx[VEC], vy[VEC], gx[VEC], gy[VEC], vl[VEC], gl[VEC], c1[VEC], g1[VEC], c2[VEC], g2[VEC];
            if (d_up) {
                bins_load<DT, VEC>(up_raw, up0 + i, vx); bins_load<DT, VEC>(up_raw, up0 + units + i, vy);
                bins_load_f32<VEC>(g_up, up0 + i, gx); bins_load_f32<VEC>(g_up, up0 + units + i, gy);
            }
            if (d_lat) { bins_load<DT, VEC>(lat_raw, px0 + i, vl); bins_load_f32<VEC>(g_lat, px0 + i, gl); }
            if (d_upc) { bins_load<DT, VEC>(up_lc, px0 + i, c1); bins_load_f32<VEC>(g_upc, px0 + i, g1); }
            if (d_latc) { bins_load<DT, VEC>(lat_lc, px0 + i, c2); bins_load_f32<VEC>(g_latc, px0 + i, g2); }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                if (d_up) {
                    const float n = sqrtf(vx[k] * vx[k] + vy[k] * vy[k]);      // the forward's expression
                    const float ux = vx[k] / n, uy = vy[k] / n;
                    const float c = (ux * gy[k] - uy * gx[k]) / n;
                    const bool clamped = n < 1e-12f;
                    vx[k] = clamped ? gx[k] / 1e-12f : -uy * c;
                    vy[k] = clamped ? gy[k] / 1e-12f : ux * c;
                }
                if (d_lat) {
                    const float t = tanhf(vl[k]), e = expf(-fabsf(vl[k]));
                    vl[k] = (t < -1.0f + 1e-5f || t > 1.0f - 1e-5f) ? 0.0f : gl[k] * (2.0f * e / (1.0f + e * e));
                }
                if (d_upc) { const float e = expf(-fabsf(c1[k])); c1[k] = g1[k] * (e / ((1.0f + e) * (1.0f + e))); }
                if (d_latc) { const float e = expf(-fabsf(c2[k])); c2[k] = g2[k] * (e / ((1.0f + e) * (1.0f + e))); }
            }
            if (d_up) { pack_store_grad<DT, VEC>(d_up, up0 + i, vx); pack_store_grad<DT, VEC>(d_up, up0 + units + i, vy); }
            if (d_lat) pack_store_grad<DT, VEC>(d_lat, px0 + i, vl);
            if (d_upc) pack_store_grad<DT, VEC>(d_upc, px0 + i, c1);
            if (d_latc) pack_store_grad<DT, VEC>(d_latc, px0 + i, c2);
        }
    }
}

// ---------------------------------------------------------------- classification heads (the same step, the other format)
// UpDecoder / LatitudeDecoder with loss_type == "classification" (the original PerspectiveFields weights): the heads emit
// Ku and Kl logits per pixel, the fields are the decodes of the per-pixel argmax.  ONE pass reads the Ku + Kl logit planes
// once and writes the planes the sweep reads; a decode has one value per bin, so it is a gather from the caller's tables
// (include/gclm.h: gclm_pack_fields_bins), staged in LDS once per workgroup -- no device cos or sin, the reference's bits.
// Lanes run along pixels and the channel loop runs inside the lane: every channel read is a row of consecutive pixels, the
// running maximum and its index never leave registers.  DT = the logits' type (gclm_logit_dtype); VEC = pixels per lane:
// one 16-byte load per channel (4 floats, 8 halves) where the planes allow it, else 1.
// slat: sin of the latitude just written, by the sweep's polynomial, as in pack_fields_kernel; a bin centre lies strictly
// inside +-pi/2, so no range fold here either.
// torch.argmax's rule over the K planes of one image: the first index of the greatest value; a NaN is greater than everything
// and the first NaN wins; all -inf gives 0.  A later x replaces the best only if the best is no NaN and x <= best is false.
template <int DT, int VEC>
__device__ __forceinline__ void bins_argmax(const bins_elem<DT>* __restrict__ logits, int K, size_t N, size_t i, int (&idx)[VEC]) {
    float best[VEC], v[kBinsUnroll][VEC];
    bins_load<DT, VEC>(logits, i, best);
#pragma unroll
    for (int k = 0; k < VEC; ++k) idx[k] = 0;
    auto take = [&](const float (&x)[VEC], int c) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const bool t = !(x[k] <= best[k]) && best[k] == best[k];
            best[k] = t ? x[k] : best[k];
            idx[k] = t ? c : idx[k];
        }
    };
    int c = 1;
    for (; c + kBinsUnroll <= K; c += kBinsUnroll) {
#pragma unroll
        for (int u = 0; u < kBinsUnroll; ++u) bins_load<DT, VEC>(logits + (size_t)(c + u) * N, i, v[u]);
#pragma unroll
        for (int u = 0; u < kBinsUnroll; ++u) take(v[u], c + u);
    }
    for (; c < K; ++c) {
        bins_load<DT, VEC>(logits + (size_t)c * N, i, v[0]);
        take(v[0], c);
    }
}
// (the log-confidences may be their own outputs, lane by lane: no __restrict__ on those four)
template <int DT, int VEC>
__global__ __launch_bounds__(256) void pack_bins_kernel(const bins_elem<DT>* __restrict__ up_logits, int Ku,
                                                        const bins_elem<DT>* __restrict__ lat_logits, int Kl,
                                                        const float* __restrict__ up_table, const float* __restrict__ lat_table,
                                                        const float* up_lc, const float* lat_lc, int B, size_t N,
                                                        float* __restrict__ up, float* upc, float* __restrict__ lat, float* latc,
                                                        float* __restrict__ slat) {
    extern __shared__ float bins_tab[];      // (Ku, 2) then (Kl)
    float* const ltab = bins_tab + 2 * Ku;
    for (int t = threadIdx.x; t < 2 * Ku; t += blockDim.x) bins_tab[t] = up_table[t];
    for (int t = threadIdx.x; t < Kl; t += blockDim.x) ltab[t] = lat_table[t];
    __syncthreads();
    const size_t units = N / VEC;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const bins_elem<DT>* ul = up_logits + (size_t)b * Ku * N;
        const bins_elem<DT>* ll = lat_logits + (size_t)b * Kl * N;
        float* ox = up + (size_t)b * 2 * N;
        const size_t plane = (size_t)b * N / VEC;      // in units: N is a multiple of VEC
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += (size_t)gridDim.x * blockDim.x) {
            int ub[VEC], lb[VEC];
            bins_argmax<DT, VEC>(ul, Ku, N, i, ub);
            bins_argmax<DT, VEC>(ll, Kl, N, i, lb);
            float vx[VEC], vy[VEC], vl[VEC], c[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                vx[k] = bins_tab[2 * ub[k]];
                vy[k] = bins_tab[2 * ub[k] + 1];
                vl[k] = ltab[lb[k]];
            }
            bins_store_f32<VEC>(ox, i, vx);
            bins_store_f32<VEC>(ox + N, i, vy);
            bins_store_f32<VEC>(lat, plane + i, vl);
            if (slat) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) c[k] = dev::sin_halfpi(vl[k]);
                bins_store_f32<VEC>(slat, plane + i, c);
            }
            if (up_lc) {
                bins_load_f32<VEC>(up_lc, plane + i, c);
#pragma unroll
                for (int k = 0; k < VEC; ++k) c[k] = 1.0f / (1.0f + expf(-c[k]));      // pack_fields_kernel's expression
                bins_store_f32<VEC>(upc, plane + i, c);
            }
            if (lat_lc) {
                bins_load_f32<VEC>(lat_lc, plane + i, c);
#pragma unroll
                for (int k = 0; k < VEC; ++k) c[k] = 1.0f / (1.0f + expf(-c[k]));
                bins_store_f32<VEC>(latc, plane + i, c);
            }
        }
    }
}

// ---------------------------------------------------------------- _post_process (the step after the path)
// GeoCalib._post_process (extractor.py:51-69) brings the fields back to the input resolution with
// F.interpolate(mode="bilinear", align_corners=False); one launch for any number of (h, w) planes of up to 8 tensors.
// Source index as in ATen (area_pixel_compute_source_index): src = max(0, (dst + 0.5) * in/out - 0.5).
// Every path below evaluates, per output value and with these roundings,
//     top/bot = fma(r[x0], 1 - lx, r[x1] * lx)        out = fma(top, 1 - ly, bot * ly)
// so the scalar, gather and window kernels agree bit for bit (test_upsample_paths_agree_bitwise).
__device__ __forceinline__ float up_src(int X, float scale) { return fmaxf(__fmaf_rn((float)X + 0.5f, scale, -0.5f), 0.f); }
__device__ __forceinline__ float up_lerp(float a, float b, float l) { return __fmaf_rn(a, 1.f - l, __fmul_rn(b, l)); }

// Scalar path: any width / alignment; one output value per thread and iteration, rows walked with an incremental
// (row, column) counter instead of a division per pixel.
__device__ __forceinline__ void upsample_plane(const float* __restrict__ s, float* __restrict__ d, int h, int w, int H, int W) {
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const unsigned units = (unsigned)H * (unsigned)W;
    const unsigned stride = gridDim.x * blockDim.x;
    const int dY = (int)(stride / (unsigned)W), dX = (int)(stride - (unsigned)dY * (unsigned)W);
    unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
    int Y = (int)(q / (unsigned)W), X = (int)(q - (unsigned)Y * (unsigned)W);
    for (; q < units; q += stride) {
        const float fy = up_src(Y, sy);
        const int y0 = min((int)fy, h - 1), y1 = min(y0 + 1, h - 1);
        const float ly = fy - (float)y0;
        const float* r0 = s + (size_t)y0 * w;
        const float* r1 = s + (size_t)y1 * w;
        const float fx = up_src(X, sx);
        const int x0 = min((int)fx, w - 1), x1 = min(x0 + 1, w - 1);
        const float lx = fx - (float)x0;
        d[(size_t)Y * W + X] = up_lerp(up_lerp(r0[x0], r0[x1], lx), up_lerp(r1[x0], r1[x1], lx), ly);
        Y += dY; X += dX;
        if (X >= W) { X -= W; ++Y; }
    }
}

// float4 paths (W % 4 == 0, 16-byte aligned planes).  A WAVE owns 64 float4 units (256 output pixels, ONE 1 KiB
// non-temporal store per output row: the output is the traffic, it is written once and read by a later kernel).
//   * The wave index is made scalar (readfirstlane): row terms and the row-reuse branches are SALU, not exec-masked VALU.
//   * WINDOW (upsampling by >= 1.5 horizontally, w >= 4): the eight taps of a lane's four pixels lie within FOUR consecutive
//     source floats, so a source row costs ONE 16-byte load per lane (4-byte aligned) and the horizontal interpolation is
//     a 5-term FMA chain over that window with per-lane weights -- 10 v_pk_fma_f32; round 4 used 24 v_cmp + 24 v_cndmask
//     register selects.  Descending order makes the chain reproduce up_lerp exactly: every other term is an exact zero,
//     the last non-zero term fused is the x0 tap; E carries the clamped right edge (x1 == x0, both weights on t.w).
//   * Position q of a row maps to unit (q + o) mod Wu, o = the units from the row's first byte up to the next 128-byte
//     line: every full wave store then starts on a line.  Rows of 1620 floats (6480 B) are not whole lines; round 4
//     wrote each wave's 1 KiB across nine lines, two of them partial, and the stores alone took 1.75x a flat fill
//     (profiles/archive/r05_upsample_bench.log: 652 -> 439 us for 64 x 5 planes 320x480 -> 1080x1620).
//   * CONSEC (rows are whole 64-byte half lines, Wu % 4 == 0): a wave walks ROWS consecutive output rows; every source
//     row it needs is loaded up front (RMAX, when the vertical ratio bounds their number) and its horizontally interpolated
//     values stay in registers for all output rows that tap it.  The (up to four) waves of a block take adjacent strips
//     of the same rows, so that a block writes whole rows.
//   * PHASED (ragged rows): rows 8 apart share the phase o (8 Wu = 0 mod 8 units), so wave i of a 512-thread block owns
//     rows Y0 + i + 8 j and keeps its column weights; all 2 ROWS window loads are issued before the arithmetic.
//   * GATHER (any other ratio): per-lane dword gathers, consecutive rows, no rotation.
typedef float up_v2 __attribute__((ext_vector_type(2)));
typedef float up_v4 __attribute__((ext_vector_type(4)));
typedef float up_v4u __attribute__((ext_vector_type(4), aligned(4)));
// NW = 4: upsampling by >= 1.5 (above).  NW = 5: upsampling by 1 ... 1.5 -- four adjacent outputs then tap at most FIVE
// consecutive source floats (one 16-byte + one 4-byte load per source row and lane, a 6-term chain); GeoCalib resizes
// the short side to 320 px, so every input between 320 and 480 px on its short side lands here.
template <int NW>
struct UpCol {
    int xs, u;               // window start (source floats), output unit of this lane
    up_v2 W[NW][2], E[2];    // weight of window float j for the outputs (0, 1) and (2, 3)
    bool live;
};
template <int NW>
struct UpWin { float t[NW]; };
template <int NW>
__device__ __forceinline__ UpWin<NW> up_load_window(const float* p) {
    UpWin<NW> r;
    const up_v4u q = *reinterpret_cast<const up_v4u*>(p);
    r.t[0] = q.x; r.t[1] = q.y; r.t[2] = q.z; r.t[3] = q.w;
    if constexpr (NW == 5) r.t[4] = p[4];
    return r;
}
template <int NW>
__device__ __forceinline__ UpCol<NW> up_col_weights(int q, int o, int w, int W, float sx) {
    UpCol<NW> c;
    const int Wu = W >> 2;
    int u = q + (Wu >= 64 ? o : 0);      // rows shorter than one wave store: nothing to align
    if (u >= Wu) u -= Wu;
    c.live = q < Wu;
    if (!c.live) u = 0;
    c.u = u;
    int x0[4], x1[4];
    float lx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float fx = up_src(u * 4 + k, sx);
        x0[k] = min((int)fx, w - 1);
        x1[k] = min(x0[k] + 1, w - 1);
        lx[k] = fx - (float)x0[k];
    }
    c.xs = min(x0[0], w - NW);
    float Wm[NW][4], Em[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i0 = x0[k] - c.xs, i1 = x1[k] - c.xs;
#pragma unroll
        for (int j = 0; j < NW; ++j) Wm[j][k] = (j == i1) ? lx[k] : ((j == i0) ? 1.f - lx[k] : 0.f);
        Em[k] = (i0 == i1) ? 1.f - lx[k] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) { c.W[j][0] = up_v2{Wm[j][0], Wm[j][1]}; c.W[j][1] = up_v2{Wm[j][2], Wm[j][3]}; }
    c.E[0] = up_v2{Em[0], Em[1]}; c.E[1] = up_v2{Em[2], Em[3]};
    return c;
}
template <int NW>
__device__ __forceinline__ void up_hwindow(const UpCol<NW>& c, const UpWin<NW>& t, up_v2 (&o)[2]) {
#pragma unroll
    for (int hlf = 0; hlf < 2; ++hlf) {
        const float last = t.t[NW - 1];
        up_v2 a = up_v2{last, last} * c.W[NW - 1][hlf];
        a = __builtin_elementwise_fma(up_v2{last, last}, c.E[hlf], a);
#pragma unroll
        for (int j = NW - 2; j >= 0; --j) a = __builtin_elementwise_fma(up_v2{t.t[j], t.t[j]}, c.W[j][hlf], a);
        o[hlf] = a;
    }
}
struct UpRow { int y0, y1; float ly; };
__device__ __forceinline__ UpRow up_row_terms(int Y, int h, float sy) {      // Y wave-uniform: the results are scalars
    const float fy = up_src(Y, sy);
    const int y0 = min((int)fy, h - 1);
    UpRow r;
    r.ly = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, fy - (float)y0)));
    r.y0 = __builtin_amdgcn_readfirstlane(y0);
    r.y1 = min(r.y0 + 1, h - 1);
    return r;
}
__device__ __forceinline__ void up_vblend_store(float* p, bool live, float ly, const up_v2 (&ha)[2], const up_v2 (&hb)[2]) {
    const up_v2 l2 = up_v2{ly, ly}, m2 = up_v2{1.f - ly, 1.f - ly};
    const up_v2 o0 = __builtin_elementwise_fma(ha[0], m2, hb[0] * l2), o1 = __builtin_elementwise_fma(ha[1], m2, hb[1] * l2);
    if (live) __builtin_nontemporal_store(up_v4{o0.x, o0.y, o1.x, o1.y}, reinterpret_cast<up_v4*>(p));
}
__device__ __forceinline__ unsigned up_line_unit(const float* d) { return (unsigned)((reinterpret_cast<uintptr_t>(d) >> 4) & 7u); }

// RMAX > 0: the rows Y0 .. Y0 + ROWS - 1 tap at most RMAX source rows (the host derives it from the vertical ratio),
// all loaded before the arithmetic; RMAX = 0: loaded as the walk reaches them (vertical downsampling).
template <int ROWS, int NW, int RMAX>
__device__ __forceinline__ void upsample_consec(const float* __restrict__ s, float* __restrict__ d, int h, int w, int H, int W, int q,
                                                int Y0) {
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const UpCol<NW> c = up_col_weights<NW>(q, (int)((8u - up_line_unit(d)) & 7u), w, W, sx);
    const int Yend = min(Y0 + ROWS, H);
    const float* sc = s + c.xs;
    float* dc = d + c.u * 4;
    if constexpr (RMAX > 0) {
        const UpRow ra = up_row_terms(Y0, h, sy), rb = up_row_terms(Yend - 1, h, sy);
        const int ylo = ra.y0, yhi = rb.y1, n = yhi - ylo + 1;
        UpWin<NW> t[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) t[r] = up_load_window<NW>(sc + (size_t)min(ylo + r, yhi) * w);
        up_v2 hc[2], hn[2];
        up_hwindow<NW>(c, t[0], hc);
        int Y = Y0;
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            if (r < n) {
                if (r + 1 < RMAX && r + 1 < n) up_hwindow<NW>(c, t[r + 1 < RMAX ? r + 1 : r], hn);
                else { hn[0] = hc[0]; hn[1] = hc[1]; }        // y1 == y0: the last source row
                while (Y < Yend) {
                    const UpRow rt = up_row_terms(Y, h, sy);
                    if (rt.y0 - ylo != r) break;
                    up_vblend_store(dc + (size_t)Y * W, c.live, rt.ly, hc, hn);
                    ++Y;
                }
                hc[0] = hn[0]; hc[1] = hn[1];
            }
        }
    } else {
        int ya = -1, yb = -1;
        up_v2 ha[2] = {up_v2{0.f, 0.f}, up_v2{0.f, 0.f}}, hb[2] = {up_v2{0.f, 0.f}, up_v2{0.f, 0.f}};
        for (int Y = Y0; Y < Yend; ++Y) {
            const UpRow rt = up_row_terms(Y, h, sy);
            if (!(rt.y0 == ya && rt.y1 == yb)) {
                if (rt.y0 == yb) { ha[0] = hb[0]; ha[1] = hb[1]; }
                else if (rt.y0 != ya) up_hwindow<NW>(c, up_load_window<NW>(sc + (size_t)rt.y0 * w), ha);
                ya = rt.y0;
                if (rt.y1 == rt.y0) { hb[0] = ha[0]; hb[1] = ha[1]; }
                else up_hwindow<NW>(c, up_load_window<NW>(sc + (size_t)rt.y1 * w), hb);
                yb = rt.y1;
            }
            up_vblend_store(dc + (size_t)Y * W, c.live, rt.ly, ha, hb);
        }
    }
}
template <int ROWS, int NW>
__device__ __forceinline__ void upsample_phased(const float* __restrict__ s, float* __restrict__ d, int h, int w, int H, int W, int q,
                                                int Ya) {
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const unsigned g = up_line_unit(d) + (unsigned)Ya * (unsigned)(W >> 2);      // the row's first unit, mod 8 = its phase
    const UpCol<NW> c = up_col_weights<NW>(q, (int)((8u - (g & 7u)) & 7u), w, W, sx);
    const float* sc = s + c.xs;
    float* dc = d + c.u * 4;
    UpWin<NW> ta[ROWS], tb[ROWS];
    UpRow rt[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        rt[j] = up_row_terms(min(Ya + 8 * j, H - 1), h, sy);
        ta[j] = up_load_window<NW>(sc + (size_t)rt[j].y0 * w);
        tb[j] = up_load_window<NW>(sc + (size_t)rt[j].y1 * w);
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        up_v2 ha[2], hb[2];
        up_hwindow<NW>(c, ta[j], ha);
        up_hwindow<NW>(c, tb[j], hb);
        const int Y = Ya + 8 * j;
        up_vblend_store(dc + (size_t)Y * W, c.live && Y < H, rt[j].ly, ha, hb);
    }
}
template <int ROWS>
__device__ __forceinline__ void upsample_gather(const float* __restrict__ s, float* __restrict__ d, int h, int w, int H, int W, int Xu,
                                                int Y0) {
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const bool live = Xu * 4 < W;
    int x0[4], x1[4];
    float lx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float fx = up_src(min(Xu * 4 + k, W - 1), sx);
        x0[k] = min((int)fx, w - 1);
        x1[k] = min(x0[k] + 1, w - 1);
        lx[k] = fx - (float)x0[k];
    }
    auto hrow = [&](int y, float (&o)[4]) {
        const float* r = s + (size_t)y * w;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = up_lerp(r[x0[k]], r[x1[k]], lx[k]);
    };
    int ya = -1, yb = -1;
    float ha[4] = {0.f, 0.f, 0.f, 0.f}, hb[4] = {0.f, 0.f, 0.f, 0.f};
    const int Yend = min(Y0 + ROWS, H);
    for (int Y = Y0; Y < Yend; ++Y) {
        const UpRow rt = up_row_terms(Y, h, sy);
        if (!(rt.y0 == ya && rt.y1 == yb)) {
            if (rt.y0 == yb) {
#pragma unroll
                for (int k = 0; k < 4; ++k) ha[k] = hb[k];
            } else if (rt.y0 != ya) {
                hrow(rt.y0, ha);
            }
            ya = rt.y0;
            if (rt.y1 == rt.y0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) hb[k] = ha[k];
            } else {
                hrow(rt.y1, hb);
            }
            yb = rt.y1;
        }
        if (live)
            __builtin_nontemporal_store(up_v4{up_lerp(ha[0], hb[0], rt.ly), up_lerp(ha[1], hb[1], rt.ly), up_lerp(ha[2], hb[2], rt.ly),
                                              up_lerp(ha[3], hb[3], rt.ly)},
                                        reinterpret_cast<up_v4*>(d + (size_t)Y * W + Xu * 4));
    }
}

// grid = (strips of 64 units, row groups, planes of all tensors); blockIdx.z strides over the planes beyond 65 535
struct UpPlane { const float* s; float* d; };
__device__ __forceinline__ UpPlane up_plane(const UpsampleMulti& m, int P, int h, int w, int H, int W) {
    int t = 0;
    while (t < m.n - 1 && P >= m.planes[t]) { P -= m.planes[t]; ++t; }
    return UpPlane{m.src[t] + (size_t)P * h * w, m.dst[t] + (size_t)P * H * W};
}
enum { kUpScalar = 0, kUpGather = 1, kUpConsec = 2, kUpPhased = 3 };
template <int KIND, int ROWS, int NW, int RMAX>
__global__ __launch_bounds__(KIND == kUpPhased ? 512 : 256) void upsample_kernel(UpsampleMulti m, int total, int h, int w, int H, int W,
                                                                                  int rowblock) {
    if constexpr (KIND == kUpScalar) {
        for (int P = blockIdx.y; P < total; P += gridDim.y) {
            const UpPlane pl = up_plane(m, P, h, w, H, W);
            upsample_plane(pl.s, pl.d, h, w, H, W);
        }
    } else {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        // CONSEC: the waves of a block take ADJACENT strips of the same ROWS rows -- a block writes whole rows (of up to
        // 1024 px), row after row, instead of four row groups of one strip: 0.346 -> 0.323 ms on the x2 case
        // (profiles/archive/r05_upsample_bench.log, "rowblock").  The other kinds: blockIdx.x = strip, waves = row groups / phases.
        // (one image: the old grouping, four row groups of one strip per block -- 4.5 against 5.5 us for 5 planes of 480x640)
        const bool rb = KIND == kUpConsec && rowblock != 0;
        const int strip = rb ? blockIdx.x * 4 + wave : blockIdx.x;
        const int q = strip * 64 + (threadIdx.x & 63);
        const int Y0 = KIND == kUpPhased ? blockIdx.y * (8 * ROWS) + wave : (rb ? blockIdx.y * ROWS : (blockIdx.y * 4 + wave) * ROWS);
        if (Y0 >= H || strip * 64 >= (W >> 2)) return;
        for (int P = blockIdx.z; P < total; P += gridDim.z) {
            const UpPlane pl = up_plane(m, P, h, w, H, W);
            if constexpr (KIND == kUpGather) upsample_gather<ROWS>(pl.s, pl.d, h, w, H, W, q, Y0);
            else if constexpr (KIND == kUpPhased) upsample_phased<ROWS, NW>(pl.s, pl.d, h, w, H, W, q, Y0);
            else upsample_consec<ROWS, NW, RMAX>(pl.s, pl.d, h, w, H, W, q, Y0);
        }
    }
}
// A window of NW source floats holds every tap of four adjacent output pixels when x0[3] <= x0[0] + NW - 2, i.e.
// 3 sx <= NW - 2 in exact arithmetic (NW = 4: upsampling by >= 1.5; NW = 5: by >= 1).  The kernel derives x0 from fp32
// (X + 0.5) sx - 0.5, whose error per value is below fx 2^-23 <= w 2^-23; two of them must not bridge the gap
// (NW - 2) - 3 w / W = ((NW - 2) W - 3 w) / W, so away from the exact ratios (1.5: no source coordinate of a lane's first
// pixel is an integer, (16 u - 1) / 6; 1: every coordinate is an exact integer) the window path needs gap 2^21 > w W.
__host__ inline bool upsample_window_ok(int nw, int w, int W) {
    const long long gap = (long long)(nw - 2) * W - 3LL * w;
    return w >= nw && (gap == 0 || (gap > 0 && (double)gap * 2097152.0 > (double)w * (double)W));
}
struct UpPlan { int kind, nw, pref; };      // pref: 0 none, 1 = 3 h <= 2 H (2 ROWS / 3 + 3 source rows), 2 = h <= H (ROWS + 2)
__host__ inline UpPlan upsample_plan(const UpsampleMulti& m, int h, int w, int H, int W) {
    bool vec4 = W % 4 == 0;
    for (int t = 0; t < m.n; ++t) vec4 = vec4 && (reinterpret_cast<uintptr_t>(m.dst[t]) & 15u) == 0;
    if (!vec4) return UpPlan{kUpScalar, 4, 0};
    const int nw = upsample_window_ok(4, w, W) ? 4 : (upsample_window_ok(5, w, W) ? 5 : 0);
    if (!nw) return UpPlan{kUpGather, 4, 0};
    // Ragged = rows that are not a whole number of 64-BYTE half lines (W / 4 units of 16 B, not divisible by 4): only then do
    // the wave stores of the consecutive-row kernel leave 16 ... 48-byte slivers.  Rows of 2240 B (560 px) alternate between
    // line-aligned and 64 B off, and stream at full rate without rotation (5.9 TB/s against 4.0 through the phased kernel,
    // which gives up the vertical reuse); rows of 6480 B (1620 px) need it (3.9 against 5.6).
    if ((W / 4) % 4 != 0) return UpPlan{kUpPhased, nw, 0};
    return UpPlan{kUpConsec, nw, 3LL * h <= 2LL * H ? 1 : (h <= H ? 2 : 0)};
}
}  // namespace

// Several tensors of (h, w) planes in ONE launch (the four tensors _post_process resizes: up 2 planes per image, latitude,
// two confidences): a single-image calibrate() pays one launch instead of four.  Small jobs (one image) take half the
// rows per wave: twice the waves to fill 256 CUs.
template <int KIND, int NW, int PREF>
static void launch_upsample_kind(const UpsampleMulti& m, int total, int h, int w, int H, int W, bool small, hipStream_t s) {
    const int strips = (W / 4 + 63) / 64, gz = total < 65535 ? total : 65535;
    auto go = [&](auto rows) {
        constexpr int R = decltype(rows)::value;
        constexpr int RMAX = PREF == 1 ? 2 * R / 3 + 3 : (PREF == 2 ? R + 2 : 0);
        if (KIND == kUpConsec && !small) {
            const int waves = strips < 4 ? strips : 4;            // 640 px: 2.5 strips = 3 waves per block, no idle wave
            hipLaunchKernelGGL((upsample_kernel<KIND, R, NW, RMAX>), dim3((strips + 3) / 4, (H + R - 1) / R, gz), dim3(64 * waves), 0, s, m, total,
                               h, w, H, W, 1);
        } else {
            const dim3 grid(strips, KIND == kUpPhased ? (H + 8 * R - 1) / (8 * R) : (H + 4 * R - 1) / (4 * R), gz);
            hipLaunchKernelGGL((upsample_kernel<KIND, R, NW, RMAX>), grid, dim3(KIND == kUpPhased ? 512 : 256), 0, s, m, total, h, w, H, W, 0);
        }
    };
    // one image: half the rows per wave, twice the waves for 256 CUs; the phased five-float window with 8 rows holds 16
    // windows = 138 VGPRs, one 512-thread block per CU: 4 rows (90 VGPRs, two blocks) stream faster
    if (small || (KIND == kUpPhased && NW == 5)) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, 8>{});
}
hipError_t launch_upsample_multi(const UpsampleMulti& m, int h, int w, int H, int W, hipStream_t s) {
    long long total = 0;
    for (int t = 0; t < m.n; ++t) total += m.planes[t];
    if (total == 0 || (size_t)H * W == 0) return hipSuccess;
    if (total > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool small = (double)total * H * W < 16.0e6;
    const int n = (int)total;
    const UpPlan p = upsample_plan(m, h, w, H, W);
    if (p.kind == kUpScalar) {
        unsigned bx = ((unsigned)H * (unsigned)W + 256 * 4 - 1) / (256 * 4);
        hipLaunchKernelGGL((upsample_kernel<kUpScalar, 1, 4, 0>), dim3(bx < 1 ? 1 : bx, (unsigned)(total < 65535 ? total : 65535)), dim3(256), 0, s, m, n,
                           h, w, H, W, 0);
    } else if (p.kind == kUpGather) {
        launch_upsample_kind<kUpGather, 4, 0>(m, n, h, w, H, W, small, s);
    } else if (p.kind == kUpPhased) {
        if (p.nw == 4) launch_upsample_kind<kUpPhased, 4, 0>(m, n, h, w, H, W, small, s);
        else launch_upsample_kind<kUpPhased, 5, 0>(m, n, h, w, H, W, small, s);
    } else if (p.nw == 4) {
        if (p.pref == 1) launch_upsample_kind<kUpConsec, 4, 1>(m, n, h, w, H, W, small, s);
        else if (p.pref == 2) launch_upsample_kind<kUpConsec, 4, 2>(m, n, h, w, H, W, small, s);
        else launch_upsample_kind<kUpConsec, 4, 0>(m, n, h, w, H, W, small, s);
    } else {
        if (p.pref == 1) launch_upsample_kind<kUpConsec, 5, 1>(m, n, h, w, H, W, small, s);
        else if (p.pref == 2) launch_upsample_kind<kUpConsec, 5, 2>(m, n, h, w, H, W, small, s);
        else launch_upsample_kind<kUpConsec, 5, 0>(m, n, h, w, H, W, small, s);
    }
    return hipGetLastError();
}
hipError_t launch_upsample(const float* src, int planes, int h, int w, int H, int W, float* dst, hipStream_t s) {
    UpsampleMulti m{};
    m.src[0] = src; m.dst[0] = dst; m.planes[0] = planes; m.n = 1;
    return launch_upsample_multi(m, h, w, H, W, s);
}

hipError_t launch_pack_fields(const float* up_raw, const float* up_lc, const float* lat_raw, const float* lat_lc,
                              int B, int H, int W, bool vec4, float* up, float* upc, float* lat, float* latc,
                              float* slat, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    const size_t N = (size_t)H * W;
    const size_t units = vec4 ? N / 4 : N;
    // one unit per thread and image where the image allows (one pass: +3 % over 128 blocks walking a grid-stride loop)
    const int bx = (int)((units + 255) / 256 < 2048 ? (units + 255) / 256 : 2048);
    const dim3 grid(bx, B < 4096 ? B : 4096), block(256);
    if (vec4) hipLaunchKernelGGL(pack_fields_kernel<4>, grid, block, 0, s, up_raw, up_lc, lat_raw, lat_lc, B, N, up, upc, lat, latc, slat);
    else hipLaunchKernelGGL(pack_fields_kernel<1>, grid, block, 0, s, up_raw, up_lc, lat_raw, lat_lc, B, N, up, upc, lat, latc, slat);
    return hipGetLastError();
}

// The grid of the two typed epilogue passes: pack_fields' own.
static dim3 pack_grid(size_t units, int B) {
    const int bx = (int)((units + 255) / 256 < 2048 ? (units + 255) / 256 : 2048);
    return dim3(bx, B < 4096 ? B : 4096);
}
// 16-bit raws (float32 raws are launch_pack_fields').  `vec`: as below.
hipError_t launch_pack_fields_typed(int dtype, const void* up_raw, const void* up_lc, const void* lat_raw, const void* lat_lc, int B,
                                    int H, int W, bool vec, float* up, float* upc, float* lat, float* latc, float* slat, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    const size_t N = (size_t)H * W;
    auto go = [&](auto dt, auto v) {
        constexpr int DT = decltype(dt)::value, VEC = decltype(v)::value;
        using E = bins_elem<DT>;
        hipLaunchKernelGGL((pack_fields_kernel<VEC, DT>), pack_grid(N / VEC, B), dim3(256), 0, s, static_cast<const E*>(up_raw),
                           static_cast<const E*>(up_lc), static_cast<const E*>(lat_raw), static_cast<const E*>(lat_lc), B, N, up, upc, lat,
                           latc, slat);
    };
    auto width = [&](auto dt) {
        if (vec) go(dt, std::integral_constant<int, 8>{});
        else go(dt, std::integral_constant<int, 1>{});
    };
    if (dtype == GCLM_LOGITS_F16) width(std::integral_constant<int, GCLM_LOGITS_F16>{});
    else if (dtype == GCLM_LOGITS_BF16) width(std::integral_constant<int, GCLM_LOGITS_BF16>{});
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_pack_fields_backward(int dtype, const void* up_raw, const void* up_lc, const void* lat_raw, const void* lat_lc, int B,
                                       int H, int W, bool vec, const float* g_up, const float* g_upc, const float* g_lat,
                                       const float* g_latc, void* d_up, void* d_upc, void* d_lat, void* d_latc, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    const size_t N = (size_t)H * W;
    auto go = [&](auto dt, auto v) {
        constexpr int DT = decltype(dt)::value, VEC = decltype(v)::value;
        using E = bins_elem<DT>;
        hipLaunchKernelGGL((pack_fields_backward_kernel<DT, VEC>), pack_grid(N / VEC, B), dim3(256), 0, s, static_cast<const E*>(up_raw),
                           static_cast<const E*>(up_lc), static_cast<const E*>(lat_raw), static_cast<const E*>(lat_lc), B, N, g_up, g_upc,
                           g_lat, g_latc, static_cast<E*>(d_up), static_cast<E*>(d_upc), static_cast<E*>(d_lat), static_cast<E*>(d_latc));
    };
    auto width = [&](auto dt) {
        if (vec) go(dt, std::integral_constant<int, bins_vec(decltype(dt)::value)>{});
        else go(dt, std::integral_constant<int, 1>{});
    };
    if (dtype == GCLM_LOGITS_F32) width(std::integral_constant<int, GCLM_LOGITS_F32>{});
    else if (dtype == GCLM_LOGITS_F16) width(std::integral_constant<int, GCLM_LOGITS_F16>{});
    else if (dtype == GCLM_LOGITS_BF16) width(std::integral_constant<int, GCLM_LOGITS_BF16>{});
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// `vec`: every plane of the call is 16-byte aligned and H * W is a multiple of the type's pixels per lane (the entry decides).
template <int DT, int VEC>
static void launch_pack_bins_as(const void* up_logits, int Ku, const void* lat_logits, int Kl, const float* up_table,
                                const float* lat_table, const float* up_lc, const float* lat_lc, int B, size_t N, float* up,
                                float* upc, float* lat, float* latc, float* slat, hipStream_t s) {
    const size_t units = N / VEC;
    const int bx = (int)((units + 255) / 256 < 2048 ? (units + 255) / 256 : 2048);
    const dim3 grid(bx, B < 4096 ? B : 4096), block(256);
    hipLaunchKernelGGL((pack_bins_kernel<DT, VEC>), grid, block, (size_t)(2 * Ku + Kl) * sizeof(float), s,
                       static_cast<const bins_elem<DT>*>(up_logits), Ku, static_cast<const bins_elem<DT>*>(lat_logits), Kl, up_table,
                       lat_table, up_lc, lat_lc, B, N, up, upc, lat, latc, slat);
}
hipError_t launch_pack_fields_bins(const void* up_logits, int Ku, const void* lat_logits, int Kl, int dtype, const float* up_table,
                                   const float* lat_table, const float* up_lc, const float* lat_lc, int B, int H, int W, bool vec,
                                   float* up, float* upc, float* lat, float* latc, float* slat, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    const size_t N = (size_t)H * W;
    auto go = [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (vec) launch_pack_bins_as<DT, bins_vec(DT)>(up_logits, Ku, lat_logits, Kl, up_table, lat_table, up_lc, lat_lc, B, N, up, upc, lat, latc, slat, s);
        else launch_pack_bins_as<DT, 1>(up_logits, Ku, lat_logits, Kl, up_table, lat_table, up_lc, lat_lc, B, N, up, upc, lat, latc, slat, s);
    };
    if (dtype == GCLM_LOGITS_F32) go(std::integral_constant<int, GCLM_LOGITS_F32>{});
    else if (dtype == GCLM_LOGITS_F16) go(std::integral_constant<int, GCLM_LOGITS_F16>{});
    else if (dtype == GCLM_LOGITS_BF16) go(std::integral_constant<int, GCLM_LOGITS_BF16>{});
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace gclm
