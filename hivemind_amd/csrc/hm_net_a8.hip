// hm_net_a8.hip — the RISEv3 forward on native FP8 MFMA (e4m3 activations and weights) as ONE gfx950 kernel launch: the __global__
// form of narrow_position_a8 (hm_net_a8_device.hpp) and its launch, behind the hm_net handle of hm_net.hip (hm_net_create_a8).  The
// grid and the row loop are those of the narrow fp16 form.  A translation unit of its own, built like hm_net_w8.hip without packed
// fp32 VALU operations: the scale-and-bias epilogues and the quantisation steps stay single-lane operations, rounding as written.
#include <hip/hip_runtime.h>

#include "hm_net_a8_device.hpp"
#include "hm_net_a8.hpp"

namespace hmn {

template <int CTILES, bool K5>
__global__ __launch_bounds__(512, 1) void rise_forward_a8(const NetDescA8* __restrict__ ndp, const uint8_t* __restrict__ w8, const h16* __restrict__ wh,
                                                          const float* __restrict__ wf, const h16* __restrict__ planes, int n, int copMax, int uBytes,
                                                          h16* __restrict__ value, h16* __restrict__ piA, h16* __restrict__ piB,
                                                          h16* __restrict__ wdl, h16* __restrict__ ml,
                                                          const int* __restrict__ groupRows, int group, unsigned long long* __restrict__ clk) {
    if (clk && threadIdx.x == 0) atomicMin(clk, (unsigned long long)__builtin_amdgcn_s_memrealtime());   // leg clock: (start, end) pair
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const NetDescA8& nd = *ndp;
    for (int sIdx = blockIdx.x; sIdx < n; sIdx += gridDim.x) {
        if (groupRows && (sIdx % group) >= groupRows[sIdx / group]) continue;
        narrow_position_a8<CTILES, K5>(nd, w8, wh, wf, planes + (size_t)sIdx * HM_PLANE_VALUES, (size_t)sIdx, copMax, uBytes, smem, value, piA, piB, wdl, ml);
    }
    if (clk && threadIdx.x == 0) atomicMax(clk + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

// applies `f` to the instantiation for a trunk of C channels
template <typename F>
static hipError_t with_a8(int C, bool k5, F f) {
    if (C == 128) return k5 ? f(rise_forward_a8<4, true>) : f(rise_forward_a8<4, false>);
    if (C == 384) return k5 ? f(rise_forward_a8<12, true>) : f(rise_forward_a8<12, false>);
    return hipErrorInvalidValue;
}

hipError_t a8_set_lds(int C, bool k5, size_t ldsBytes) {
    return with_a8(C, k5, [&](auto kern) { return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes); });
}

hipError_t a8_launch(const A8Launch& a, int grid, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                     void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_clk) {
    return with_a8(a.C, a.k5, [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), a.ldsBytes, st, static_cast<const NetDescA8*>(a.d_nd), static_cast<const uint8_t*>(a.d_w8),
                           static_cast<const h16*>(a.d_wh), static_cast<const float*>(a.d_wf), static_cast<const h16*>(d_planes), n, a.copMax, a.uBytes,
                           static_cast<h16*>(d_value), static_cast<h16*>(d_pi_a), static_cast<h16*>(d_pi_b), static_cast<h16*>(d_wdl),
                           static_cast<h16*>(d_moves_left), reinterpret_cast<const int*>(d_group_rows), group, d_clk);
        return hipGetLastError();
    });
}

}  // namespace hmn
