// hm_net_xboard.hpp — host seam between the hm_net handle (hm_net.hip) and the cross-board forward's translation unit (hm_net_xboard.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace hmn {

// what the two launches of a cross-board network need (resolved once by hm_net_create_xboard)
struct XbLaunch {
    const void* d_nd = nullptr;     // the trunk's NetDesc on the device (its value-head entries serve the tail)
    void* d_xd = nullptr;           // XbDesc on the device (owned)
    const void* d_wh = nullptr;
    const void* d_wf = nullptr;
    void* d_feat = nullptr;         // [maxRows][64][C] fp16 feature buffer between the two launches (owned)
    int C = 0, copMax = 0, uHalfs = 0, maxRows = 0;
    bool k5 = false;
    size_t ldsTrunk = 0;
};

// validates the tail descriptor (hmn::XbDesc as int32s), uploads it, allocates the feature buffer and sets both kernels' LDS limits;
// hipErrorInvalidValue + *why for an unsupported geometry
hipError_t xb_prepare(XbLaunch& a, const int32_t* desc, size_t desc_ints, const char** why);
void xb_release(XbLaunch& a);
// trunk (features form) then tail, in slices of maxRows rows, on `st`
hipError_t xb_launch(const XbLaunch& a, int maxBlocks, hipStream_t st, const void* d_planes, int n, void* d_value, void* d_pi_a, void* d_pi_b, void* d_wdl,
                     void* d_moves_left, const int32_t* d_group_rows, int group, unsigned long long* d_clk);
// the tail alone on caller-supplied features [n][64][C]
hipError_t xb_tail(const XbLaunch& a, int maxBlocks, hipStream_t st, const void* d_features, const void* d_planes, int n, void* d_value, void* d_pi_a,
                   void* d_pi_b, void* d_wdl, void* d_moves_left);

}  // namespace hmn
