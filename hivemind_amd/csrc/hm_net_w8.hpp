// hm_net_w8.hpp — host seam between the hm_net handle (hm_net.hip) and the FP8-weight forward's translation unit (hm_net_w8.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace hmn {

// what a launch of rise_forward_w8 needs of a loaded fp8 network (resolved once by hm_net_create_w8)
struct W8Launch {
    const void* d_nd = nullptr;     // NetDescW8 on the device
    const void* d_w8 = nullptr;     // e4m3 codes in fragment-pair order
    const void* d_wh = nullptr;     // fp16 parameters (stem, depthwise, ECA, value linear)
    const void* d_wf = nullptr;     // fp32 biases and scales
    int C = 0, copMax = 0, uHalfs = 0;
    bool k5 = false;
    size_t ldsBytes = 0;
};

hipError_t w8_set_lds(int C, bool k5, size_t ldsBytes);
hipError_t w8_launch(const W8Launch& a, int grid, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                     void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_dbg, unsigned long long* d_clk);

}  // namespace hmn
