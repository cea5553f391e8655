// hm_net_xboard.hip — CrossBoardRiseV3 (the reference's crossboard-risev33, src/architectures/rise_mobile_v3.py:242-412) as two launches on
// one stream: the 8-wave RISEv3 trunk in its features form (narrow_position<.., FEAT = true>: the trunk's output tile goes to a
// per-handle feature buffer instead of into the heads), then the tail kernel of hm_net_xboard_device.hpp (token projections, context
// tokens, one or two cross-attention blocks, value fusion + value head, two policy heads), one workgroup of 8 waves per position.
// The feature round trip is 48 KB per position of the 384-channel trunk.  Both launches honour the groups form and the leg clock.
#include <hip/hip_runtime.h>

#include <cstring>

#include "hm_net_xboard_device.hpp"
#include "hm_net_xboard.hpp"

namespace hmn {

// rows rowBase .. rowBase + n - 1 of the batch: feature row = local index, group membership by the batch row
template <int CTILES, bool K5>
__global__ __launch_bounds__(512, 1) void rise_features_narrow(const NetDesc* __restrict__ ndp, const h16* __restrict__ wh, const float* __restrict__ wf,
                                                               const h16* __restrict__ planes, int rowBase, int n, int copMax, int uHalfs,
                                                               h16* __restrict__ feat, const int* __restrict__ groupRows, int group,
                                                               unsigned long long* __restrict__ clk) {
    if (clk && threadIdx.x == 0) atomicMin(clk, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    int dbgN = 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const NetDesc& nd = *ndp;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int sIdx = rowBase + i;
        if (groupRows && (sIdx % group) >= groupRows[sIdx / group]) continue;
        narrow_position<CTILES, K5, false, NoPolicyEpi, true>(nd, wh, wf, planes + (size_t)sIdx * HM_PLANE_VALUES, (size_t)sIdx, copMax, uHalfs, smem,
                                                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dbgN, NoPolicyEpi(),
                                                              feat + (size_t)i * 64 * (CTILES * 32));
    }
    if (clk && threadIdx.x == 0) atomicMax(clk + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

template <int CTILES>
__global__ __launch_bounds__(512, 1) void xboard_tail_kernel(const NetDesc* __restrict__ ndp, const XbDesc* __restrict__ xdp, const h16* __restrict__ wh,
                                                             const float* __restrict__ wf, const h16* __restrict__ feat, const h16* __restrict__ planes,
                                                             int rowBase, int n, h16* __restrict__ value, h16* __restrict__ piA, h16* __restrict__ piB,
                                                             h16* __restrict__ wdl, h16* __restrict__ ml, const int* __restrict__ groupRows, int group,
                                                             unsigned long long* __restrict__ clk) {
    if (clk && threadIdx.x == 0) atomicMin(clk, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int sIdx = rowBase + i;
        if (groupRows && (sIdx % group) >= groupRows[sIdx / group]) continue;
        xboard_position<CTILES>(*ndp, *xdp, wh, wf, feat + (size_t)i * 64 * (CTILES * 32), planes + (size_t)sIdx * HM_PLANE_VALUES, (size_t)sIdx, smem,
                                value, piA, piB, wdl, ml);
    }
    if (clk && threadIdx.x == 0) atomicMax(clk + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

template <typename F>
static hipError_t with_trunk(const XbLaunch& a, F f) {
    if (a.C == 64) return a.k5 ? f(rise_features_narrow<2, true>) : f(rise_features_narrow<2, false>);
    if (a.C == 128) return a.k5 ? f(rise_features_narrow<4, true>) : f(rise_features_narrow<4, false>);
    return a.k5 ? f(rise_features_narrow<12, true>) : f(rise_features_narrow<12, false>);
}
template <typename F>
static hipError_t with_tail(const XbLaunch& a, F f) {
    if (a.C == 64) return f(xboard_tail_kernel<2>);
    if (a.C == 128) return f(xboard_tail_kernel<4>);
    return f(xboard_tail_kernel<12>);
}

hipError_t xb_prepare(XbLaunch& a, const int32_t* desc, size_t desc_ints, const char** why) {
    *why = "";
    if (desc_ints * 4 != sizeof(XbDesc)) { *why = "bad cross-board descriptor size"; return hipErrorInvalidValue; }
    XbDesc xd;
    memcpy(&xd, desc, sizeof(XbDesc));
    if (xd.C != a.C || (a.C != 64 && a.C != 128 && a.C != 384)) { *why = "cross-board tail: trunk width must be 64, 128 or 384 and match the trunk descriptor"; return hipErrorInvalidValue; }
    if (xd.layers != 1 && xd.layers != 2) { *why = "cross-board tail: one or two attention layers"; return hipErrorInvalidValue; }
    if (!(xd.eps > 0.0f)) { *why = "cross-board tail: LayerNorm eps must be positive"; return hipErrorInvalidValue; }
    if (a.maxRows <= 0) { *why = "cross-board tail: max_rows must be positive"; return hipErrorInvalidValue; }
    const unsigned hoffs[] = {xd.tp_w[0], xd.tp_w[1], xd.ph_w1[0], xd.ph_w1[1], xd.ph_w2[0], xd.ph_w2[1], xd.vf_w};
    for (unsigned o : hoffs) if (o & 7) { *why = "cross-board tail: matrix offsets must be multiples of 8 halfs"; return hipErrorInvalidValue; }
    for (int i = 0; i < xd.layers; ++i)
        if ((xd.L[i].wq | xd.L[i].wk | xd.L[i].wv | xd.L[i].wo | xd.L[i].w1 | xd.L[i].w2) & 7) { *why = "cross-board tail: matrix offsets must be multiples of 8 halfs"; return hipErrorInvalidValue; }
    hipError_t e = hipMalloc(&a.d_xd, sizeof(XbDesc));
    if (e == hipSuccess) e = hipMemcpy(a.d_xd, &xd, sizeof(XbDesc), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&a.d_feat, (size_t)a.maxRows * 64 * a.C * sizeof(h16));
    if (e == hipSuccess) e = with_trunk(a, [&](auto k) { return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.ldsTrunk); });
    if (e == hipSuccess) e = with_tail(a, [&](auto k) { return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)XB_LDS_BYTES); });
    if (e != hipSuccess) xb_release(a);
    return e;
}
void xb_release(XbLaunch& a) {
    if (a.d_xd) (void)hipFree(a.d_xd);
    if (a.d_feat) (void)hipFree(a.d_feat);
    a.d_xd = nullptr; a.d_feat = nullptr;
}

static hipError_t tail_launch(const XbLaunch& a, int grid, hipStream_t st, const void* feat, const void* d_planes, int rowBase, int n, void* d_value, void* d_pi_a,
                              void* d_pi_b, void* d_wdl, void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_clk) {
    return with_tail(a, [&](auto k) {
        hipLaunchKernelGGL(k, dim3(grid), dim3(512), XB_LDS_BYTES, st, static_cast<const NetDesc*>(a.d_nd), static_cast<const XbDesc*>(a.d_xd),
                           static_cast<const h16*>(a.d_wh), static_cast<const float*>(a.d_wf), static_cast<const h16*>(feat), static_cast<const h16*>(d_planes),
                           rowBase, n, static_cast<h16*>(d_value), static_cast<h16*>(d_pi_a), static_cast<h16*>(d_pi_b), static_cast<h16*>(d_wdl),
                           static_cast<h16*>(d_moves_left), reinterpret_cast<const int*>(d_group_rows), group, d_clk);
        return hipGetLastError();
    });
}

hipError_t xb_launch(const XbLaunch& a, int maxBlocks, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                     void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_clk) {
    for (int base = 0; base < n; base += a.maxRows) {
        const int rows = n - base < a.maxRows ? n - base : a.maxRows, grid = rows < maxBlocks ? rows : maxBlocks;
        hipError_t e = with_trunk(a, [&](auto k) {
            hipLaunchKernelGGL(k, dim3(grid), dim3(512), a.ldsTrunk, st, static_cast<const NetDesc*>(a.d_nd), static_cast<const h16*>(a.d_wh),
                               static_cast<const float*>(a.d_wf), static_cast<const h16*>(d_planes), base, rows, a.copMax, a.uHalfs,
                               static_cast<h16*>(a.d_feat), reinterpret_cast<const int*>(d_group_rows), group, d_clk);
            return hipGetLastError();
        });
        if (e == hipSuccess) e = tail_launch(a, grid, st, a.d_feat, d_planes, base, rows, d_value, d_pi_a, d_pi_b, d_wdl, d_moves_left, d_group_rows, group, d_clk);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t xb_tail(const XbLaunch& a, int maxBlocks, hipStream_t st, const void* d_features, const void* d_planes, int n, void* d_value, void* d_pi_a,
                   void* d_pi_b, void* d_wdl, void* d_moves_left) {
    // rowBase = 0 and n rows: feature row i belongs to batch row i
    return tail_launch(a, n < maxBlocks ? n : maxBlocks, st, d_features, d_planes, 0, n, d_value, d_pi_a, d_pi_b, d_wdl, d_moves_left, nullptr, 0, nullptr);
}

}  // namespace hmn
