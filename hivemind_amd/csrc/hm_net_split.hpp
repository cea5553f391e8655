// hm_net_split.hpp — host seam between the hm_net handle (hm_net.hip) and the team form's translation unit (hm_net_split.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace hmn {

// what a launch of rise_forward_split needs of a loaded fp16 network with a 384-channel trunk (resolved by hm_net_set_split)
struct SplitLaunch {
    const void* d_nd = nullptr;     // NetDesc on the device
    const void* d_wh = nullptr;     // packed fp16 parameters
    const void* d_wf = nullptr;     // fp32 biases
    int T = 0;                      // team size: 2 or 3
    bool k5 = false;
    size_t ldsBytes = 0;
    int teamsMax = 0;               // teams that are resident together: floor(min(occupancy x CUs, maxBlocks) / T)
    int yHalfs = 0;                 // halfs of one team's Y region (hm_net_split_device.hpp: workspace layout)
    void* ws = nullptr;             // workspace, owned by the handle
};

// Sets the kernel's LDS size, sizes the teams from the occupancy of the instantiation with that LDS, the CU count of the current device
// and `maxBlocks`, and allocates and zeroes the workspace for a network whose widest block has maxCop expanded channels.
// hipErrorInvalidValue: not even one team is resident.
hipError_t split_prepare(SplitLaunch& a, int maxCop, int maxBlocks);
void split_release(SplitLaunch& a);
hipError_t split_launch(const SplitLaunch& a, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                        void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_clk);
// blocking: waits for the device, reads the error word and, when it is set, zeroes it together with every team's counters
hipError_t split_take_error(const SplitLaunch& a, int* code);

}  // namespace hmn
