// hm_net_pair.hpp — host seam between the hm_net handle (hm_net.hip) and the pair form's translation unit (hm_net_pair.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace hmn {

// what a launch of rise_forward_pair needs of a loaded fp16 network (resolved by hm_net_set_pair)
struct PairLaunch {
    const void* d_nd = nullptr;     // NetDesc on the device
    const void* d_wh = nullptr;     // packed fp16 parameters
    const void* d_wf = nullptr;     // fp32 biases
    int C = 0, copMax = 0, uPos = 0;   // uPos: halfs of ONE position's union region
    bool k5 = false;
    size_t ldsBytes = 0;
};

// The pair form's LDS plan for a trunk of C channels (64 or 128) whose widest block has maxCop expanded channels: the largest chunk
// (a multiple of 64 channels, or maxCop itself) that fits 160 KiB.  False when even a 64-channel chunk does not fit.
bool pair_plan(int C, int cinPad, int maxCop, PairLaunch& out);
hipError_t pair_set_lds(const PairLaunch& a);
hipError_t pair_launch(const PairLaunch& a, int maxBlocks, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                       void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_dbg, unsigned long long* d_clk);

}  // namespace hmn
