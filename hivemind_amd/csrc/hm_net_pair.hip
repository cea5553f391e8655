// hm_net_pair.hip — the pair form of the fused RISEv3 forward as ONE gfx950 kernel launch: the __global__ form of pair_position
// (hm_net_pair_device.hpp: two positions per 4-wave workgroup, M = 128 rows per weight fragment), its LDS plan and its launch, behind
// the hm_net handle of hm_net.hip (hm_net_set_pair).  A translation unit of its own, so that the object code and register allocation
// of the one-position kernels stay as they are.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>

#include "hm_net_pair_device.hpp"
#include "hm_net_pair.hpp"
#include "hm_net_plan.hpp"

namespace hmn {

// Workgroup iteration p takes rows 2p and 2p + 1.  A row is live when it lies inside the batch and inside its group's row count; a pair
// without a live row is skipped, a pair with one computes it (the dead position runs on the live row's planes and stores nothing).
template <int CTILES, bool K5>
__global__ __launch_bounds__(256, 1) void rise_forward_pair(const NetDesc* __restrict__ ndp, const h16* __restrict__ wh, const float* __restrict__ wf,
                                                            const h16* __restrict__ planes, int n, int copMax, int uPos,
                                                            h16* __restrict__ value, h16* __restrict__ piA, h16* __restrict__ piB,
                                                            h16* __restrict__ wdl, h16* __restrict__ ml,
                                                            const int* __restrict__ groupRows, int group,
                                                            unsigned long long* __restrict__ dbg, unsigned long long* __restrict__ clk) {
    if (clk && threadIdx.x == 0) atomicMin(clk, (unsigned long long)__builtin_amdgcn_s_memrealtime());   // leg clock: (start, end) pair
    int dbgN = 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const NetDesc& nd = *ndp;
    auto live = [&](int r) { return r < n && (!groupRows || (r % group) < groupRows[r / group]); };
    for (int r0 = 2 * blockIdx.x; r0 < n; r0 += 2 * gridDim.x) {
        const bool st[2] = {live(r0), live(r0 + 1)};
        if (!st[0] && !st[1]) continue;
        const size_t row[2] = {(size_t)r0, (size_t)r0 + 1};
        const h16* const pin[2] = {planes + row[st[0] ? 0 : 1] * HM_PLANE_VALUES, planes + row[st[1] ? 1 : 0] * HM_PLANE_VALUES};
        pair_position<CTILES, K5>(nd, wh, wf, pin, row, st, copMax, uPos, smem, value, piA, piB, wdl, ml, dbg, dbgN);
    }
    if (clk && threadIdx.x == 0) atomicMax(clk + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

// applies `f` to the instantiation for a trunk of C channels
template <typename F>
static hipError_t with_pair(int C, bool k5, F f) {
    if (C == 64) return k5 ? f(rise_forward_pair<2, true>) : f(rise_forward_pair<2, false>);
    if (C == 128) return k5 ? f(rise_forward_pair<4, true>) : f(rise_forward_pair<4, false>);
    return hipErrorInvalidValue;
}

bool pair_plan(int C, int cinPad, int maxCop, PairLaunch& out) {
    // narrow_lds_plan with the per-position parts doubled; the union regions state the ECA's 32 x C partial sums as a tenant
    const NarrowLdsPlan pl = narrow_lds_plan(C, cinPad, maxCop, 2, (size_t)32 * C * 2);
    if (!pl.ok) return false;
    out.C = C; out.copMax = pl.copMax; out.uPos = pl.uHalfs; out.ldsBytes = pl.ldsBytes;
    return true;
}

hipError_t pair_set_lds(const PairLaunch& a) {
    return with_pair(a.C, a.k5, [&](auto kern) { return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.ldsBytes); });
}

hipError_t pair_launch(const PairLaunch& a, int maxBlocks, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                       void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_dbg, unsigned long long* d_clk) {
    const int grid = std::min((n + 1) / 2, maxBlocks);
    return with_pair(a.C, a.k5, [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), a.ldsBytes, st, static_cast<const NetDesc*>(a.d_nd), static_cast<const h16*>(a.d_wh),
                           static_cast<const float*>(a.d_wf), static_cast<const h16*>(d_planes), n, a.copMax, a.uPos,
                           static_cast<h16*>(d_value), static_cast<h16*>(d_pi_a), static_cast<h16*>(d_pi_b), static_cast<h16*>(d_wdl),
                           static_cast<h16*>(d_moves_left), reinterpret_cast<const int*>(d_group_rows), group, d_dbg, d_clk);
        return hipGetLastError();
    });
}

}  // namespace hmn
