// gclm_logits.h -- planes of float32, float16 or bfloat16 elements: what the typed kernels share -- the head epilogue, its
// backward and the classification heads' decode (gclm_fields.hip), and the classification heads' loss (gclm_bin_loss.hip).
// DT = the elements' type (gclm_logit_dtype); VEC = pixels per lane: one 16-byte access per plane (4 floats, 8 halves) where the
// planes allow it, else 1.  (the names are the classification heads', which had them first)
#pragma once
#include <type_traits>

#include "gclm_internal.h"

namespace gclm {

typedef uint32_t bins_u4 __attribute__((ext_vector_type(4)));
typedef float bins_f4 __attribute__((ext_vector_type(4)));
template <int DT>
using bins_elem = std::conditional_t<DT == GCLM_LOGITS_F32, float, uint16_t>;
constexpr int bins_vec(int dt) { return dt == GCLM_LOGITS_F32 ? 4 : 8; }
constexpr int kBinsUnroll = 8;      // pack_bins_kernel, bin_loss_kernel: channel loads in flight per lane

// 16-bit logits widen to float exactly, so one comparison serves the three types
template <int DT>
__device__ __forceinline__ float bins_widen(uint32_t bits) {      // a float's 32 bits, or a half's 16 in the low half
    if constexpr (DT == GCLM_LOGITS_F32) return __builtin_bit_cast(float, bits);
    else if constexpr (DT == GCLM_LOGITS_BF16) return __builtin_bit_cast(float, bits << 16);
    else return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}
// the values of one channel at the VEC pixels of unit i
template <int DT, int VEC>
__device__ __forceinline__ void bins_load(const bins_elem<DT>* __restrict__ plane, size_t i, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = bins_widen<DT>((uint32_t)__builtin_bit_cast(std::conditional_t<DT == GCLM_LOGITS_F32, uint32_t, uint16_t>,
                                                           __builtin_nontemporal_load(plane + i)));
    } else {
        const bins_u4 q = __builtin_nontemporal_load(reinterpret_cast<const bins_u4*>(plane) + i);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if constexpr (DT == GCLM_LOGITS_F32) v[k] = bins_widen<DT>(w[k]);
            else v[k] = bins_widen<DT>((k & 1) ? w[k >> 1] >> 16 : w[k >> 1] & 0xffffu);
        }
    }
}

template <int DT>
__device__ __forceinline__ bins_elem<DT> pack_narrow(float v) {      // round to nearest even, as torch's .to(dtype)
    if constexpr (DT == GCLM_LOGITS_F32) return v;
    else if constexpr (DT == GCLM_LOGITS_F16) return __builtin_bit_cast(uint16_t, (_Float16)v);
    else {
        const uint32_t u = __builtin_bit_cast(uint32_t, v);
        return v != v ? (uint16_t)0x7fc0u : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}

}  // namespace gclm
