// hm_net_plan.hpp — host side of the narrow forms' LDS layout (the carve-up at the top of narrow_position, hm_net_device.hpp, which its
// sibling bodies repeat): the one plan that sizes it and picks the chunk of expanded channels, and the one walk over a descriptor's
// blocks for its widest expansion.
//   Xs[65][C+8] per position | union region per position { Ss[65][max(C, cin_pad)+8] , Y1[chunk][66] + Y2[64][chunk+8] } |
//   b1[chunk] b2[chunk] b3[C] | depthwise taps [chunk][25] | per position: ECA / head scratch [4][C] + [C] + 64 floats
#pragma once
#include <algorithm>
#include <cstdlib>
#include <string>

namespace hmn {

constexpr size_t NARROW_LDS_LIMIT = 160 * 1024;                         // one CU's LDS

struct NarrowLdsPlan {
    bool ok;
    int copMax, uHalfs;                                                  // expanded channels kept in LDS at a time; halfs of one position's union region
    size_t ldsBytes;
};
// maxCop: the widest expansion of the network; positions: positions per workgroup (2: the pair form — tiles, union regions and ECA /
// head scratch per position, the chunk's parameters once); extraUnionHalfs: another tenant the union region must hold (the pair form
// states the ECA's [32][C] floats); copCap > 0: an upper bound of the chunk.  A network whose expansions do not fit is walked in chunks
// of a multiple of 64 channels; HM_NET_COP_CHUNK overrides the chunk (measurements).  ok = false: not even 64 channels fit.
inline NarrowLdsPlan narrow_lds_plan(int C, int cinPad, int maxCop, int positions, size_t extraUnionHalfs, int copCap = 0) {
    const size_t ldx = C + 8, ldi = cinPad + 8, P = positions;
    auto bytes_for = [&](int cm) {
        size_t u = std::max({(size_t)cm * 66 + (size_t)64 * (cm + 8), (size_t)65 * std::max(ldx, ldi), extraUnionHalfs});
        u = (u + 7) & ~(size_t)7;
        return std::make_pair(u, P * (65 * ldx + u) * 2 + (2 * (size_t)cm + C) * 4 + ((((size_t)cm * 25 + 7) & ~(size_t)7) * 2) + P * (5 * (size_t)C + 64) * 4);
    };
    int copMax = std::max(32, maxCop);
    if (const char* ce = std::getenv("HM_NET_COP_CHUNK")) copMax = std::max(64, std::atoi(ce) & ~63);
    if (copCap > 0 && copMax > copCap) copMax = copCap;
    if (positions > 1 && copMax > 64 && bytes_for(copMax).second > NARROW_LDS_LIMIT) copMax &= ~63;   // (the pair form's rule: its chunks are multiples of 64)
    while (copMax > 64 && bytes_for(copMax).second > NARROW_LDS_LIMIT) copMax -= 64;
    const auto ub = bytes_for(copMax);
    return {ub.second <= NARROW_LDS_LIMIT, copMax, (int)ub.first, ub.second};
}

// The plan of the forward on native FP8 MFMA (the carve-up at the top of narrow_position_a8, hm_net_a8_device.hpp), in bytes:
//   Xs[64][C+8] fp16 | Xq[65][C+16] codes | union region { input staging [65][cin_pad+8] fp16 , Ss[65][C+16] codes ,
//   Y1[chunk][66] fp16 + Y2[64][chunk+16] codes , ECA partial sums [32][C] + [4][C] floats } | b1 b2 s1 [chunk] b3[C] |
//   depthwise taps [chunk][25] | gates [C] + head scratch [64] floats
// Y2, Ss and the GEMMs' copy of x as bytes pay for Xq: the 384-channel trunk keeps the fp16 forms' chunk of 320 channels.  The chunk is
// a multiple of 64 (one k-step of the FP8 MFMA).
struct A8LdsPlan {
    bool ok;
    int copMax, uBytes;
    size_t ldsBytes;
};
// minUnion: another tenant the union region must hold; tailBytes: LDS the caller keeps behind the layout (counted against the limit,
// not part of ldsBytes)
inline A8LdsPlan a8_lds_plan(int C, int cinPad, int maxCop, size_t minUnion = 0, size_t tailBytes = 0) {
    const size_t ldx = C + 8, ldq = C + 16, ldi = cinPad + 8;
    auto bytes_for = [&](int cm) {
        size_t u = std::max({(size_t)cm * 132 + (size_t)64 * (cm + 16), 65 * ldq, 65 * ldi * 2, (size_t)36 * C * 4, minUnion});
        u = (u + 15) & ~(size_t)15;
        return std::make_pair(u, 64 * ldx * 2 + 65 * ldq + u + (3 * (size_t)cm + C) * 4 + ((((size_t)cm * 25 + 7) & ~(size_t)7) * 2) + ((size_t)C + 64) * 4);
    };
    int copMax = (std::max(64, maxCop) + 63) & ~63;
    if (const char* ce = std::getenv("HM_NET_COP_CHUNK")) copMax = std::min(copMax, std::max(64, std::atoi(ce) & ~63));   // (measurements, tests)
    while (copMax > 64 && bytes_for(copMax).second + tailBytes > NARROW_LDS_LIMIT) copMax -= 64;
    const auto ub = bytes_for(copMax);
    return {ub.second + tailBytes <= NARROW_LDS_LIMIT, copMax, (int)ub.first, ub.second};
}
// The plan of the same layout for the serve form (narrow_position_a8<.., WT>: the evaluator role of the single-launch search): the
// policy staging Pol[160][64] fp16 and the prior pipeline's scratch (stagingBytes together) lie behind Sq[65][C+16] inside the union
// region, which is enlarged to hold them where the expansion's tenants leave it smaller (narrow trunks, or a small chunk); behind the
// layout the evaluator role keeps its 16-byte item word.  The 384-channel trunk at its chunk of 320: 26 000 + 36 928 of 63 744 bytes.
struct A8ServePlan {
    bool ok;
    int copMax, uBytes, polOff;                                          // polOff: bytes from the start of the union region to Pol
    size_t ldsBytes;
};
inline A8ServePlan a8_serve_plan(int C, int cinPad, int maxCop, size_t stagingBytes) {
    const size_t polOff = (65 * ((size_t)C + 16) + 15) & ~(size_t)15;
    const A8LdsPlan pl = a8_lds_plan(C, cinPad, maxCop, polOff + stagingBytes, 16);
    return {pl.ok, pl.copMax, pl.uBytes, (int)polOff, pl.ldsBytes};
}

// max(32, the widest `cop` of nd's blocks); requireMultipleOf32: a cop that is no positive multiple of 32 is refused (-1, *err set,
// prefixed with the form's name)
template <typename ND>
inline int max_cop(const ND& nd, bool requireMultipleOf32, const char* form, std::string* err) {
    int m = 32;
    for (int i = 0; i < nd.nblocks; ++i) {
        if (requireMultipleOf32 && (nd.blk[i].cop <= 0 || nd.blk[i].cop % 32)) {
            *err = std::string(form) + ": expanded channels must be a positive multiple of 32";
            return -1;
        }
        m = std::max(m, nd.blk[i].cop);
    }
    return m;
}

}  // namespace hmn
