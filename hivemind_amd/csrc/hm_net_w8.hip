// hm_net_w8.hip — the RISEv3 forward with FP8 (e4m3) weights as ONE gfx950 kernel launch: the __global__ form of
// narrow_position_w8 (hm_net_w8_device.hpp) and its launch, behind the hm_net handle of hm_net.hip (hm_net_create_w8).
// A translation unit of its own: it is built without packed fp32 VALU operations (Makefile: W8FLAGS), so that the epilogues'
// acc * scale + bias over sixteen accumulators stay single-lane multiplies and adds, rounding exactly as written.
#include <hip/hip_runtime.h>

#include "hm_net_w8_device.hpp"
#include "hm_net_w8.hpp"

namespace hmn {

template <int CTILES, bool K5>
__global__ __launch_bounds__(256, 1) void rise_forward_w8(const NetDescW8* __restrict__ ndp, const uint8_t* __restrict__ w8, const h16* __restrict__ wh,
                                                          const float* __restrict__ wf, const h16* __restrict__ planes, int n, int copMax, int uHalfs,
                                                          h16* __restrict__ value, h16* __restrict__ piA, h16* __restrict__ piB,
                                                          h16* __restrict__ wdl, h16* __restrict__ ml,
                                                          const int* __restrict__ groupRows, int group,
                                                          unsigned long long* __restrict__ dbg, unsigned long long* __restrict__ clk) {
    if (clk && threadIdx.x == 0) atomicMin(clk, (unsigned long long)__builtin_amdgcn_s_memrealtime());   // leg clock: (start, end) pair
    int dbgN = 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const NetDescW8& nd = *ndp;
    for (int sIdx = blockIdx.x; sIdx < n; sIdx += gridDim.x) {
        if (groupRows && (sIdx % group) >= groupRows[sIdx / group]) continue;
        narrow_position_w8<CTILES, K5>(nd, w8, wh, wf, planes + (size_t)sIdx * HM_PLANE_VALUES, (size_t)sIdx, copMax, uHalfs, smem, value, piA, piB, wdl, ml, dbg, dbgN);
    }
    if (clk && threadIdx.x == 0) atomicMax(clk + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

// applies `f` to the instantiation for a trunk of C channels
template <typename F>
static hipError_t with_w8(int C, bool k5, F f) {
    if (C == 64) return k5 ? f(rise_forward_w8<2, true>) : f(rise_forward_w8<2, false>);
    if (C == 128) return k5 ? f(rise_forward_w8<4, true>) : f(rise_forward_w8<4, false>);
    if (C == 384) return k5 ? f(rise_forward_w8<12, true>) : f(rise_forward_w8<12, false>);
    return hipErrorInvalidValue;
}

hipError_t w8_set_lds(int C, bool k5, size_t ldsBytes) {
    return with_w8(C, k5, [&](auto kern) { return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes); });
}

hipError_t w8_launch(const W8Launch& a, int grid, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                     void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_dbg, unsigned long long* d_clk) {
    return with_w8(a.C, a.k5, [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), a.ldsBytes, st, static_cast<const NetDescW8*>(a.d_nd), static_cast<const uint8_t*>(a.d_w8),
                           static_cast<const h16*>(a.d_wh), static_cast<const float*>(a.d_wf), static_cast<const h16*>(d_planes), n, a.copMax, a.uHalfs,
                           static_cast<h16*>(d_value), static_cast<h16*>(d_pi_a), static_cast<h16*>(d_pi_b), static_cast<h16*>(d_wdl),
                           static_cast<h16*>(d_moves_left), reinterpret_cast<const int*>(d_group_rows), group, d_dbg, d_clk);
        return hipGetLastError();
    });
}

}  // namespace hmn
