// gclm_hypotheses.hip -- gclm_hypothesis_scores: which of N candidate calibrations per image fits the image's predicted
// perspective fields best, in one pass over the planes (the scoring half of the reference's RANSAC baseline,
// siclib/models/optimization/ransac.py: check_up_inliers, check_latitude_inliers, get_best_index -- per hypothesis the
// confidence-weighted inlier sum of both fields, then an argmax -- with the hypotheses' fields evaluated per pixel in
// registers instead of 2 000 rendered fields per image).
//
// Per pixel and hypothesis, e_up and e_lat are the errors of gclm_field_errors (gclm_render.h: persp_up normalised /
// persp_lat at the hypothesis' camera and gravity, up_error_deg with its mask, |lat - t_lat| 180 / pi); then
//   up[b, n]  = sum_px (e_up < up_threshold ? 1 : 0) * (c_up * mask),   lat[b, n] likewise,   strict comparisons,
//   total     = up_weight up + lat_weight lat,      best[b] = the first index of the largest total.
// hit * conf is a multiplication, as in torch: a NaN error hits nothing and adds 0 (so a hypothesis with a NaN camera or
// gravity scores 0), a NaN confidence makes the sums of that field of that image NaN for every hypothesis (an infinite one
// gives NaN wherever a hypothesis misses that pixel, 0 * inf).  A NULL confidence and a NULL mask count as 1.
//
// Layout: the tile walk of gclm_render.h ("The tile walk": tile geometry, pixels per lane, wave sum, chain sum) -- a wave
// walks 64 PX adjacent pixels of a row, 4 waves cover 4 rows -- with grid = (tiles of one image, chunks of K hypotheses, B).  A block
// loads its pixels ONCE (prediction, confidence x mask: 5 PX registers), then walks its chunk: the eleven numbers of a
// hypothesis are wave-uniform and come through scalar loads (the index is built from blockIdx and the loop counter alone),
// the per-hypothesis terms (1 / fx, 1 / fy) and per-row terms (PerspRow's v, v^2, p_y) are formed once per hypothesis, before the
// pixels of the lane.  The parts of up_error_deg that depend on the prediction alone (|p|^2, the mask) do not change in
// the loop and are hoisted by the compiler.  A lane sums its PX pixels in float32, the wave sums its lanes with wave_sum
// (every lane the same bits), lane 0 leaves the pair (up, lat) of hypothesis k in LDS; after ONE barrier the block adds the
// 4 waves in order and writes 2 K floats, contiguous, into the caller's workspace:
//   rec[((b chunks + c) tiles + t) 2 K + 2 k + field]
// hypothesis_finish_kernel (grid = B, 1024 threads) then sums each hypothesis' records in float64 in a fixed order -- record
// t goes to chain t % 8, one thread per (hypothesis, chain), the chains added in order --, forms total in float64 from the
// float64 sums, rounds once, writes scores (B, N, 3) and takes the argmax of the rounded totals (NaN is the maximum, the
// lower index wins a tie).  No atomics, no block waits on another.  The bits of scores[b, n] depend on image b's pixels,
// H, W, the pixels per lane and hypothesis (b, n)'s eleven numbers alone: a hypothesis' sums never meet another
// hypothesis', and neither the chunk it falls into nor its place in the chunk enters its arithmetic.
//
// Each plane of an image is read once per chunk of K hypotheses (and mostly from L2: the chunks of one tile are adjacent in
// the grid).  K = 16, include/gclm.h: GCLM_HYPOTHESIS_CHUNK (a build with -DGCLM_HYPOTHESIS_CHUNK=8 or 32 is the measured
// alternative).  64-bit offsets.  No scratch.
#include "gclm_render.h"

namespace gclm {
namespace {

constexpr int K = GCLM_HYPOTHESIS_CHUNK;
constexpr int kChains = 8;                    // summation chains per hypothesis of the second launch
constexpr int kFinishBlock = 1024;
constexpr int kFinishChunks = kFinishBlock / (kChains * K);     // chunks one pass of the finish block covers
static_assert(K >= 1 && (K & (K - 1)) == 0 && 2 * K <= kBlock && kFinishChunks >= 1, "the chunk is a power of two of at most 128");

struct HypArgs {
    const float *cam, *grav, *up, *lat, *upc, *latc, *mask;
    float* rec;
    int N, H, W, tiles_x;
    float thr_up, thr_lat;
};

template <int MODEL, int PX>
__global__ __launch_bounds__(kBlock) void hypothesis_kernel(const HypArgs a) {
    __shared__ float s_part[kTileRows][2 * K];
    int x, y;
    const bool in = tile_pixel<PX>(a.tiles_x, a.H, a.W, x, y);
    const int chunk = blockIdx.y, b = blockIdx.z, wave = threadIdx.x >> 6;
    // the lane's pixels, once: a lane outside the image weighs 0, whatever its errors come to
    float px[PX], py[PX], l[PX], wu[PX], wl[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) px[j] = py[j] = l[j] = wu[j] = wl[j] = 0.f;
    if (in) {
        // PX > 1 runs only where W % PX == 0: x is a multiple of PX, so x + PX <= W
        const size_t hw = (size_t)a.H * a.W, o = (size_t)b * hw + (size_t)y * a.W + x;
        float m[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) m[j] = 1.f;
        if (a.mask) load_px<PX>(a.mask + o, m);
        if (a.up) {
            load_px<PX>(a.up + o + (size_t)b * hw, px);          // (B, 2, H, W): image b starts at 2 b H W
            load_px<PX>(a.up + o + (size_t)b * hw + hw, py);
#pragma unroll
            for (int j = 0; j < PX; ++j) wu[j] = 1.f;
            if (a.upc) load_px<PX>(a.upc + o, wu);
#pragma unroll
            for (int j = 0; j < PX; ++j) wu[j] *= m[j];
        }
        if (a.lat) {
            load_px<PX>(a.lat + o, l);
#pragma unroll
            for (int j = 0; j < PX; ++j) wl[j] = 1.f;
            if (a.latc) load_px<PX>(a.latc + o, wl);
#pragma unroll
            for (int j = 0; j < PX; ++j) wl[j] *= m[j];
        }
    }
    const int n0 = chunk * K, nk = a.N - n0 < K ? a.N - n0 : K;          // 1 <= nk: the grid holds no empty chunk
    for (int k = 0; k < nk; ++k) {
        // wave-uniform addresses: scalar loads
        const PerspRow r = persp_row(a.cam + ((size_t)b * a.N + (n0 + k)) * 8, a.grav + ((size_t)b * a.N + (n0 + k)) * 3, y);
        float su = 0.f, sl = 0.f;
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float u = ((float)(x + j) - r.cx) * r.ifx, r2 = u * u + r.v2;
            if (a.up) {
                const float e = up_error_deg(px[j], py[j], persp_up<MODEL>(r, u, r2, true));
                su += (e < a.thr_up ? 1.f : 0.f) * wu[j];
            }
            if (a.lat) {
                const float e = fabsf(l[j] - persp_lat<MODEL>(r, u, r2)) * kDegrees;
                sl += (e < a.thr_lat ? 1.f : 0.f) * wl[j];
            }
        }
        su = wave_sum(su), sl = wave_sum(sl);
        if ((threadIdx.x & 63) == 0) s_part[wave][2 * k] = su, s_part[wave][2 * k + 1] = sl;
    }
    __syncthreads();
    const int w = threadIdx.x;
    if (w < 2 * K) {
        float s = 0.f;                            // (the places of a last, short chunk beyond N: written, never read)
        if (w < 2 * nk) s = column_sum(s_part, w);
        a.rec[(((size_t)b * gridDim.y + chunk) * gridDim.x + blockIdx.x) * (2 * K) + w] = s;
    }
}

// Is total v at index i ahead of (bv, bi)?  A NaN is the maximum, as torch.argmax has it; equal totals: the lower index.
__device__ __forceinline__ bool ahead(float v, int i, float bv, int bi) {
    const bool nv = v != v, nb = bv != bv;
    if (nv != nb) return nv;
    if (!nv && v != bv) return v > bv;
    return i < bi;
}

// One block per image.  Thread (c, chain, k) of a pass sums the records t = chain, chain + 8, .. of hypothesis k of chunk
// c0 + c, both fields, in float64; the thread of chain 0 adds the eight chains in order, forms the total, rounds and keeps
// the best of its own hypotheses; the block then takes the best of its threads.
__global__ __launch_bounds__(kFinishBlock) void hypothesis_finish_kernel(const float* __restrict__ rec, int N, int chunks, int tiles,
                                                                         float up_weight, float lat_weight,
                                                                         float* __restrict__ scores, int* __restrict__ best) {
    __shared__ double part[kFinishChunks][kChains][2 * K];
    __shared__ float s_v[kFinishBlock / 64];
    __shared__ int s_i[kFinishBlock / 64];
    const int b = blockIdx.x, k = threadIdx.x % K, chain = (threadIdx.x / K) % kChains, cl = threadIdx.x / (K * kChains);
    float bv = -__builtin_huge_valf();
    int bi = INT32_MAX;                           // no hypothesis yet: every index is ahead of it
    for (int c0 = 0; c0 < chunks; c0 += kFinishChunks) {
        const int c = c0 + cl, n = c * K + k;
        const bool live = c < chunks && n < N;
        double acc[2] = {0.0, 0.0};                   // up, latitude (the workspace is held to 4-byte alignment only)
        if (live) chain_sum<kChains, 2>(rec + ((size_t)b * chunks + c) * tiles * (2 * K) + 2 * k, 2 * K, tiles, chain, acc);
        part[cl][chain][2 * k] = acc[0], part[cl][chain][2 * k + 1] = acc[1];
        __syncthreads();
        if (live && chain == 0) {
            const double su = column_sum(part[cl], 2 * k), sl = column_sum(part[cl], 2 * k + 1);
            const float total = (float)((double)up_weight * su + (double)lat_weight * sl);
            float* s = scores + ((size_t)b * N + n) * 3;
            s[0] = (float)su, s[1] = (float)sl, s[2] = total;
            if (ahead(total, n, bv, bi)) bv = total, bi = n;
        }
        __syncthreads();
    }
    if (!best) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ahead(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = bv, s_i[threadIdx.x >> 6] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kFinishBlock / 64; ++i)
            if (ahead(s_v[i], s_i[i], bv, bi)) bv = s_v[i], bi = s_i[i];
        best[b] = bi;
    }
}

int chunk_count(int N) { return (N + K - 1) / K; }

}  // namespace

size_t hypothesis_scores_workspace(int B, int N, int H, int W) {
    if (!call_sizes_fit(B, H, W) || N < 1 || N > kMaxCallImages) return 0;
    return tile_record_bytes((size_t)B * chunk_count(N), H, W, 2 * K, sizeof(float));
}

hipError_t launch_hypothesis_scores(int camera_model, const float* cam, const float* grav, int B, int N, int H, int W,
                                    const float* up, const float* lat, const float* upc, const float* latc, const float* mask,
                                    float up_threshold, float lat_threshold, float up_weight, float lat_weight, void* workspace,
                                    float* scores, int* best, hipStream_t st) {
    const int px = pixels_per_lane(W, {up, lat, upc, latc, mask}), tiles = tile_count(H, W, px), chunks = chunk_count(N);
    const HypArgs a{cam, grav, up, lat, upc, latc, mask, static_cast<float*>(workspace), N, H, W, tile_columns(W, px),
                    up_threshold, lat_threshold};
    return with_camera_model(camera_model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const auto kernel = with_pixels_per_lane(px, [](auto p) { return hypothesis_kernel<M, decltype(p)::value>; });
        hipLaunchKernelGGL(kernel, dim3(tiles, chunks, B), dim3(kBlock), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hypothesis_finish_kernel, dim3(B), dim3(kFinishBlock), 0, st, static_cast<const float*>(workspace), N,
                           chunks, tiles, up_weight, lat_weight, scores, best);
        return hipGetLastError();
    });
}

}  // namespace gclm
