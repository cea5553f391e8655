// hm_net_split.hip — the team form of the fused RISEv3 forward as ONE gfx950 kernel launch: the __global__ form of split_position
// (hm_net_split_device.hpp: T = 2 or 3 workgroups of 8 waves per position of the 384-channel trunk), its workspace and its launch,
// behind the hm_net handle of hm_net.hip (hm_net_set_split).  A translation unit of its own, so that the object code and register
// allocation of the one-position kernels stay as they are.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "hm_net_split_device.hpp"
#include "hm_net_split.hpp"

namespace hmn {

// Workgroup b is member b / teams of team b % teams (workgroups go round the 8 XCDs by their index, so with a multiple of 8 teams —
// 8, 16 or 64 rows — a team's members share an XCD and its L2: measured 1 - 3 % faster than neighbouring indices, which never do);
// a team takes rows team, team + teams, ...  Every member evaluates live(r) alike, so a dead row is skipped without a sync.  The grid never exceeds what is resident together (split_prepare), so every member's partners run.
template <int T, bool K5>
__global__ __launch_bounds__(512, 1) void rise_forward_split(const NetDesc* __restrict__ ndp, const h16* __restrict__ wh, const float* __restrict__ wf,
                                                             const h16* __restrict__ planes, int n,
                                                             h16* __restrict__ value, h16* __restrict__ piA, h16* __restrict__ piB,
                                                             h16* __restrict__ wdl, h16* __restrict__ ml,
                                                             const int* __restrict__ groupRows, int group,
                                                             unsigned char* ws, int teamsMax, int yHalfs, unsigned long long* __restrict__ clk) {
    if (clk && threadIdx.x == 0) atomicMin(clk, (unsigned long long)__builtin_amdgcn_s_memrealtime());   // leg clock: (start, end) pair
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const NetDesc& nd = *ndp;
    const int teams = gridDim.x / T;
    const int team = blockIdx.x % teams, m = blockIdx.x / teams;
    unsigned* sync = reinterpret_cast<unsigned*>(ws + SPLIT_WS_HEAD + SPLIT_WS_SYNC * (size_t)team);
    TeamCtx tc;
    tc.error = reinterpret_cast<unsigned*>(ws);
    tc.counter = sync;
    tc.ry = reinterpret_cast<h16*>(ws + SPLIT_WS_HEAD + SPLIT_WS_SYNC * (size_t)teamsMax) + (size_t)team * ((size_t)yHalfs + 64 * SPLIT_C);
    tc.rx = tc.ry + yHalfs;
    tc.verdict = reinterpret_cast<unsigned*>(smem + SPLIT_LDS_BYTES - 16);
    tc.stage = 0;
    // a give-up that nobody has read yet (hm_net_split_error) keeps every later launch from starting
    if (threadIdx.x == 0) *tc.verdict = __hip_atomic_load(hmq::G32(tc.error), HMQ_RLX) == 0u ? 1u : 0u;
    __syncthreads();
    bool ok = *tc.verdict != 0u;
    __syncthreads();
    auto live = [&](int r) { return !groupRows || (r % group) < groupRows[r / group]; };
    for (int r = team; ok && r < n; r += teams) {
        if (!live(r)) continue;
        ok = split_position<T, K5>(nd, wh, wf, planes + (size_t)r * HM_PLANE_VALUES, (size_t)r, m, smem, tc, value, piA, piB, wdl, ml);
    }
    // The last member to leave zeroes the team's counter for the next launch: a member leaves after its last wait, and that wait
    // returned only when every add of the launch had arrived, so nothing is in flight and nobody polls any more.  (After a give-up
    // the words are left to hm_net_split_error.)
    if (threadIdx.x == 0 && ok) {
        if (__hip_atomic_fetch_add(hmq::G32(sync + 16), 1u, HMQ_RLX) == (unsigned)T - 1u) {
            __hip_atomic_store(hmq::G32(sync), 0u, HMQ_RLX);
            __hip_atomic_store(hmq::G32(sync + 16), 0u, HMQ_RLX);
        }
    }
    if (clk && threadIdx.x == 0) atomicMax(clk + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

// applies `f` to the instantiation for a team of T
template <typename F>
static hipError_t with_split(int T, bool k5, F f) {
    if (T == 2) return k5 ? f(rise_forward_split<2, true>) : f(rise_forward_split<2, false>);
    if (T == 3) return k5 ? f(rise_forward_split<3, true>) : f(rise_forward_split<3, false>);
    return hipErrorInvalidValue;
}

static size_t ws_bytes(const SplitLaunch& a) {
    return SPLIT_WS_HEAD + (size_t)a.teamsMax * (SPLIT_WS_SYNC + ((size_t)a.yHalfs + 64 * SPLIT_C) * 2);
}

hipError_t split_prepare(SplitLaunch& a, int maxCop, int maxBlocks) {
    a.ldsBytes = SPLIT_LDS_BYTES;
    a.yHalfs = 64 * std::max(maxCop, SPLIT_C);
    int perCu = 0, dev = 0, cus = 0;
    hipError_t e = with_split(a.T, a.k5, [&](auto kern) {
        const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.ldsBytes);
        return e1 != hipSuccess ? e1 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kern, 512, a.ldsBytes);
    });
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    a.teamsMax = (int)std::min<long long>((long long)perCu * cus, maxBlocks) / a.T;
    if (a.teamsMax < 1) return hipErrorInvalidValue;
    e = hipMalloc(&a.ws, ws_bytes(a));
    if (e == hipSuccess) e = hipMemset(a.ws, 0, ws_bytes(a));
    if (e != hipSuccess) split_release(a);
    return e;
}

void split_release(SplitLaunch& a) {
    if (a.ws) (void)hipFree(a.ws);
    a.ws = nullptr;
}

hipError_t split_launch(const SplitLaunch& a, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                        void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_clk) {
    const int teams = std::min(n, a.teamsMax);
    return with_split(a.T, a.k5, [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(a.T * teams), dim3(512), a.ldsBytes, st, static_cast<const NetDesc*>(a.d_nd), static_cast<const h16*>(a.d_wh),
                           static_cast<const float*>(a.d_wf), static_cast<const h16*>(d_planes), n,
                           static_cast<h16*>(d_value), static_cast<h16*>(d_pi_a), static_cast<h16*>(d_pi_b), static_cast<h16*>(d_wdl),
                           static_cast<h16*>(d_moves_left), reinterpret_cast<const int*>(d_group_rows), group,
                           static_cast<unsigned char*>(a.ws), a.teamsMax, a.yHalfs, d_clk);
        return hipGetLastError();
    });
}

hipError_t split_take_error(const SplitLaunch& a, int* code) {
    unsigned word = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&word, a.ws, sizeof(word), hipMemcpyDeviceToHost);
    if (e == hipSuccess && word) e = hipMemset(a.ws, 0, SPLIT_WS_HEAD + SPLIT_WS_SYNC * (size_t)a.teamsMax);
    if (e == hipSuccess && word) e = hipDeviceSynchronize();
    *code = (int)word;
    return e;
}

}  // namespace hmn
