// hm_net_a8.hpp — host seam between the hm_net handle (hm_net.hip) and the translation unit of the forward on native FP8 MFMA
// (hm_net_a8.hip: e4m3 activations and weights).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace hmn {

// what a launch of rise_forward_a8 needs of a loaded network (resolved once by hm_net_create_a8)
struct A8Launch {
    const void* d_nd = nullptr;     // NetDescA8 on the device
    const void* d_w8 = nullptr;     // e4m3 codes, [K/64][tile][lane][32]
    const void* d_wh = nullptr;     // fp16 parameters (stem, depthwise, ECA, value linear)
    const void* d_wf = nullptr;     // fp32 biases, folded scales, 1 / activation scales
    int C = 0, copMax = 0, uBytes = 0;
    int cinPad = 0, maxCop = 0;     // what a8_lds_plan was given (hm_net_set_serve plans the serve form from the same)
    bool k5 = false;
    size_t ldsBytes = 0;
};

hipError_t a8_set_lds(int C, bool k5, size_t ldsBytes);
hipError_t a8_launch(const A8Launch& a, int grid, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                     void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_clk);

}  // namespace hmn
