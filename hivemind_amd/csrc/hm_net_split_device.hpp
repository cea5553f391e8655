// hm_net_split_device.hpp — the team form of the fused RISEv3 forward for the 384-channel trunk: T workgroups of 8 waves (a team,
// T = 2 or 3) carry ONE position from the input planes to the heads inside one launch, each member streaming about 1/T of every
// weight matrix.  The body of rise_forward_split (hm_net_split.hip).
//
// Work split.  No GEMM is split along K: every output element is accumulated by one wave over the same k-steps in the same order as
// in narrow_position<12, K5>, so the heads are bit-identical to the one-position forms.
//   input staging, ECA   replicated on every member (the same code on the same data); every member holds the whole tile Xs[65][C+8]
//   stem 3x3, policy trunk 3x3   member m computes its C/T output channels (12/T channel tiles x 2 square halves over 8 waves: one
//                        tile per wave with T = 3), publishes its [64][C/T] slice and gathers the others
//   mobile block         the cop/32 expanded tiles are shared by the rule [m*n/T, (m+1)*n/T).  A member runs expand -> depthwise on
//                        ITS slice in chunks of SPLIT_CM channels and publishes the depthwise output Y2; after the team has met it
//                        projects its C/T output channels over ALL cop channels in ascending order, the chunks of Y2 coming from
//                        the exchange buffer into two LDS buffers in turn; bias + residual on its channels; publish; gather
//   value head           member 0
//   policy projection    the 10 tiles (5 channel tiles x 2 square halves) shared by the same rule, stored straight to pi_a / pi_b
// That is 2 team syncs per block + stem + policy trunk = 32 per position of the deployed net.
//
// Hand-off (the rules at the top of hm_queue.hpp): bulk bytes leave with write-through stores (store16_wt); every storing wave drains;
// workgroup barrier; ONE lane adds 1 to the team's counter, polls it relaxed (s_sleep between polls) until it has reached T x stage,
// then ONE agent-scope acquire; workgroup barrier; plain loads by every wave.  The counter is monotone within a launch; the last
// member to leave the kernel zeroes it, so back-to-back launches and replays of a captured graph start from zero without a memset.
// Every spin is bounded (s_memrealtime): MEET_LIMIT_TICKS for the first wait of a launch (code 1: a partner never arrived — the team
// is not resident together), SPIN_LIMIT_TICKS for every other wait (code 2).  The spinner that gives up stores its code into the
// handle's error word and leaves; every other spinner polls that word and leaves too.
#pragma once
#include "hm_net_device.hpp"

namespace hmn {

constexpr int SPLIT_C = 384, SPLIT_LDX = SPLIT_C + 8;
constexpr int SPLIT_CM = 256;                                           // expanded channels a member keeps in LDS at a time (the chunk of the one-position form)
// union region (halfs): input staging / policy trunk Ss[65][C+8] | the ECA's [32][C] partial sums | Y1[CM][66] + Y2[64][CM+8] |
// the projection's two buffers [64][CM+8] (Y1 and Y2 are both idle by then)
constexpr int SPLIT_U_HALFS = SPLIT_CM * 66 + 64 * (SPLIT_CM + 8);
static_assert(SPLIT_U_HALFS >= 65 * SPLIT_LDX && SPLIT_U_HALFS >= 32 * SPLIT_C * 2 && SPLIT_U_HALFS >= 2 * 64 * (SPLIT_CM + 8), "union region");
static_assert(SPLIT_U_HALFS % 8 == 0 && (65 * SPLIT_LDX) % 8 == 0 && (SPLIT_CM * 66) % 8 == 0, "16-byte aligned regions");
// Xs | U | b1[CM], b2[CM], b3[C] | depthwise taps [CM][25] | ECA / head scratch | the team sync's verdict (one word)
constexpr size_t SPLIT_LDS_BYTES = (size_t)(65 * SPLIT_LDX + SPLIT_U_HALFS) * 2 + (2 * SPLIT_CM + SPLIT_C) * 4 + (((size_t)SPLIT_CM * 25 + 7) & ~(size_t)7) * 2
                                   + (5 * SPLIT_C + 64) * 4 + 16;

// Workspace of a split handle (device memory, zeroed when allocated):
//   [0, 256)                      the error word (offset 0)
//   [256 + 128 * team, + 128)     the team's counter (offset 0) and its count of members that have left the launch (offset 64)
//   then per team                 the Y region, yHalfs = 64 * max(widest cop, C) halfs, and the X region, 64 * C halfs
// Reuse of the two exchange regions.  A position writes them in the order  X: stem slices | Y: Y2 of block 0 | X: x of block 0 |
// Y: Y2 of block 1 | ... | X: x of the last block | Y: policy-trunk slices | X: the next position's stem slices.  Every write of a
// region is therefore separated from the previous READS of that region by the team sync of the OTHER region in between: a member
// writes X for block b only after it has passed the Y2 sync of block b, which completes only when every member has added to the
// counter — and a member adds after its gather of the previous X contents (program order: gather, expand, depthwise, publish Y2,
// add).  The same holds for Y: Y2 of block b + 1 is written after the x sync of block b, which every member reaches after its
// projection has read the last chunk of Y2 of block b; the trunk slices follow the last x sync; the next position's stem slices
// follow the trunk sync, which every member reaches after its last gather from X.  Writers of one region never overlap each other:
// every member owns its columns.
constexpr size_t SPLIT_WS_HEAD = 256, SPLIT_WS_SYNC = 128;
struct TeamCtx {
    h16* ry;                     // Y region: [64][cop] depthwise outputs of the current block, then [64][C] policy-trunk slices
    h16* rx;                     // X region: [64][C] stem / block outputs
    unsigned* counter;           // += 1 per member and sync; stage s is complete at T * s
    unsigned* error;             // != 0: some spin gave up, everybody leaves
    unsigned* verdict;           // LDS word: the outcome of a sync, from the polling lane to the workgroup
    unsigned stage;              // syncs this member has entered in this launch
};

// ONE lane: until *counter >= want (false: error / give-up)
__device__ __forceinline__ bool team_wait(unsigned* counter, unsigned* error, unsigned want, bool first) {
    const hmq::u64q t0 = __builtin_amdgcn_s_memrealtime();
    for (unsigned spins = 0;; ++spins) {
        if (__hip_atomic_load(hmq::G32(counter), HMQ_RLX) >= want) return true;
        __builtin_amdgcn_s_sleep(1);
        if ((spins & 63u) == 63u) {
            if (__hip_atomic_load(hmq::G32(error), HMQ_RLX)) return false;
            const hmq::u64q waited = (hmq::u64q)__builtin_amdgcn_s_memrealtime() - t0;
            if (waited > (first ? hmq::MEET_LIMIT_TICKS : hmq::SPIN_LIMIT_TICKS)) { __hip_atomic_store(hmq::G32(error), first ? 1u : 2u, HMQ_RLX); return false; }
        }
    }
}
// every thread of the member, after its write-through stores: false = the launch is given up (uniform over the workgroup)
template <int T>
__device__ __forceinline__ bool team_sync(TeamCtx& tc) {
    hmq::drain_stores();
    __syncthreads();
    ++tc.stage;
    if (threadIdx.x == 0) {
        (void)__hip_atomic_fetch_add(hmq::G32(tc.counter), 1u, HMQ_RLX);
        const bool ok = team_wait(tc.counter, tc.error, (unsigned)T * tc.stage, tc.stage == 1u);
        hmq::acquire_agent();
        *tc.verdict = ok ? 1u : 0u;
    }
    __syncthreads();
    return *tc.verdict != 0u;
}

typedef __attribute__((address_space(1))) const frag4 gfrag4c;
// columns [col, col + ncol) of a [64][*] LDS tile (pitch ldl, from column lcol) -> the same squares of an exchange region (pitch ldg,
// from column gcol), 16 bytes per lane, write-through.  ncol, the pitches and the columns are multiples of 8 halfs.
__device__ __forceinline__ void publish_cols(const h16* lds, int ldl, int lcol, h16* g, int ldg, int gcol, int ncol, int tid) {
    const int per = ncol >> 3;
    for (int i = tid; i < 64 * per; i += 512) {
        const int sq = i / per, c = (i - sq * per) * 8;
        hmq::store16_wt(g + (size_t)sq * ldg + gcol + c, *reinterpret_cast<const hmq::u32x4q*>(lds + sq * ldl + lcol + c));
    }
}
// the reverse, with plain global loads (after the team sync's acquire)
__device__ __forceinline__ void fetch_cols(h16* lds, int ldl, int lcol, const h16* g, int ldg, int gcol, int ncol, int tid) {
    const int per = ncol >> 3;
#pragma unroll 4
    for (int i = tid; i < 64 * per; i += 512) {
        const int sq = i / per, c = (i - sq * per) * 8;
        *reinterpret_cast<frag4*>(lds + sq * ldl + lcol + c) = *(gfrag4c*)(g + (size_t)sq * ldg + gcol + c);
    }
}

// Member m of a team of T: one position through the whole network.  Returns false when a team sync gave up (uniform over the
// workgroup; the outputs of the row are then unspecified).
template <int T, bool K5>
__device__ __forceinline__ bool split_position(const NetDesc& nd, const h16* __restrict__ wh, const float* __restrict__ wf, const h16* pin, size_t sIdx,
                                               int m, unsigned char* smem, TeamCtx& tc,
                                               h16* __restrict__ value, h16* __restrict__ piA, h16* __restrict__ piB, h16* __restrict__ wdl, h16* __restrict__ ml) {
    constexpr int C = SPLIT_C, ldx = SPLIT_LDX, ctiles = C / 32, CM = SPLIT_CM, NPF = HM_NPF_WIDE;
    constexpr int MT = ctiles / T, CW = MT * 32, TPW = (2 * MT + 7) / 8;   // the member's channel tiles, channels, and 32x32 tiles per wave of an N = C/T GEMM
    static_assert(ctiles % T == 0, "the channel tiles divide evenly over the team");
    h16* Xs = reinterpret_cast<h16*>(smem);                             // [65][ldx]
    h16* U = Xs + 65 * ldx;
    h16* Ss = U;                                                        // [65][ldx] (input staging uses pitch ldi)
    h16* Y1 = U;                                                        // [chunk][66]
    h16* Y2 = U + (size_t)CM * 66;                                      // [64][chunk + 8]
    float* Pf = reinterpret_cast<float*>(U + SPLIT_U_HALFS);            // b1[chunk], b2[chunk], b3[C]
    h16* Pdw = reinterpret_cast<h16*>(Pf + 2 * CM + C);                 // depthwise taps [chunk][k*k]
    float* Ev = reinterpret_cast<float*>(Pdw + (((size_t)CM * 25 + 7) & ~(size_t)7));   // ECA / head scratch: [4][C] + [C] + 64
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = 8 * (lane >> 5);
    const int stile = wave & 1;                                         // the square half of every tile this wave computes (local tile = wave + 8i)
    const int sqL = stile * 32 + (lane & 31);
    const int cbase = m * MT, c0 = cbase * 32;                          // the member's first channel tile / channel

    // ---- input planes: NCHW [74][64] fp16 -> Ss as [sq][cin_pad] (+ zero row 64); replicated
    const int ldi = nd.cin_pad + 8;
    {
        const frag4 z = {0, 0, 0, 0};
        frag4* z16 = reinterpret_cast<frag4*>(Ss);
        for (int i = tid; i < (65 * ldi) >> 3; i += 512) z16[i] = z;
    }
    for (int i = tid; i < ldx; i += 512) Xs[64 * ldx + i] = (h16)0.0f;
    __syncthreads();
    for (int c = tid; c < HM_PLANE_VALUES / 8; c += 512) {
        const half8 v = *reinterpret_cast<const half8*>(pin + 8 * c);
        const int pl = c >> 3, sq8 = (c & 7) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) Ss[(sq8 + j) * ldi + pl] = v[j];
    }
    __syncthreads();
    // ---- stem: 3x3 conv cin -> C (+bias, ReLU), the member's channels
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int lt = wave + 8 * i;
        if (lt < 2 * MT) {
            const int ctile = cbase + (lt >> 1);
            const floatx16 acc = gemm_conv3<5, false>(zero16(), Ss, sqL, ldi, 64, kh, wh + nd.stem_w, ctiles, ctile, lane);
            const int co = ctile * 32 + (lane & 31);
            const float bias = wf[nd.stem_b + co];
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) Xs[(stile * 32 + drow(rg, lane)) * ldx + co] = (h16)fmaxf(acc[rg] + bias, 0.0f);
        }
    }
    __syncthreads();
    publish_cols(Xs, ldx, c0, tc.rx, C, c0, CW, tid);
    if (!team_sync<T>(tc)) return false;
    fetch_cols(Xs, ldx, 0, tc.rx, C, 0, c0, tid);
    fetch_cols(Xs, ldx, c0 + CW, tc.rx, C, c0 + CW, C - c0 - CW, tid);
    __syncthreads();
    // ---- mobile bottleneck blocks
    for (int bi = 0; bi < nd.nblocks; ++bi) {
        const BlockDesc bd = nd.blk[bi];
        const int cop = bd.cop, kk = bd.k;
        float* sb1 = Pf; float* sb2 = Pf + CM; float* sb3 = Pf + 2 * CM;
        for (int i = tid; i < C; i += 512) sb3[i] = wf[bd.b3 + i];
        if (bd.eca) {   // x = x * hardsigmoid(W_eca . mean_sq(x) + b): replicated, the code of narrow_position
            float* part = Ev;
            float* Mv = Ev + 4 * C;
            for (int it = tid; it < 4 * C; it += 512) {
                const int c = it % C, p = it / C;
                float sacc = 0.0f;
                for (int sq = 16 * p; sq < 16 * p + 16; ++sq) sacc += (float)Xs[sq * ldx + c];
                part[p * C + c] = sacc;
            }
            __syncthreads();
            for (int c = tid; c < C; c += 512) Mv[c] = (part[c] + part[C + c] + part[2 * C + c] + part[3 * C + c]) * (1.0f / 64.0f);
            __syncthreads();
            float* part32 = reinterpret_cast<float*>(U);                // [32][C]
            {
                const h16* we = wh + bd.ecaw;                           // [ci][co]
                constexpr int CG = C >> 3, ROWS = C >> 5;
                for (int it = tid; it < 32 * CG; it += 512) {
                    const int cg = it % CG, p = it / CG;
                    float s[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                    const h16* wrow = we + (size_t)(p * ROWS) * C + 8 * cg;
                    half8 w8[ROWS];
#pragma unroll
                    for (int u = 0; u < ROWS; ++u) w8[u] = *reinterpret_cast<const half8*>(wrow + (size_t)u * C);
#pragma unroll
                    for (int u = 0; u < ROWS; ++u) {
                        const float mu = Mv[p * ROWS + u];
#pragma unroll
                        for (int k = 0; k < 8; ++k) s[k] += (float)w8[u][k] * mu;
                    }
                    float* dst = part32 + p * C + 8 * cg;
#pragma unroll
                    for (int k = 0; k < 8; ++k) dst[k] = s[k];
                }
            }
            __syncthreads();
            for (int c = tid; c < C; c += 512) {
                float sg = wf[bd.ecab + c];
#pragma unroll
                for (int p = 0; p < 32; ++p) sg += part32[p * C + c];
                Mv[c] = fminf(fmaxf(sg * (1.0f / 6.0f) + 0.5f, 0.0f), 1.0f);
            }
            __syncthreads();
            for (int i = tid; i < 32 * C; i += 512) {
                const int sq = i / (C >> 1), cc = 2 * (i - sq * (C >> 1));
                half2v* px = reinterpret_cast<half2v*>(Xs + sq * ldx + cc);
                half2v x2 = *px;
                x2[0] = (h16)((float)x2[0] * Mv[cc]); x2[1] = (h16)((float)x2[1] * Mv[cc + 1]);
                *px = x2;
            }
        }
        // the member's slice of the expanded channels: tiles [ta, tb) of cop / 32
        const int copTiles = cop >> 5;
        const int chA = (m * copTiles / T) * 32, chB = ((m + 1) * copTiles / T) * 32;
        for (int ch0 = chA; ch0 < chB; ch0 += CM) {
            const int chunk = min(CM, chB - ch0), ld2 = chunk + 8;
            for (int i = tid; i < chunk; i += 512) { sb1[i] = wf[bd.b1 + ch0 + i]; sb2[i] = wf[bd.b2 + ch0 + i]; }
            {   // depthwise taps of the chunk (ch0 and chunk are multiples of 32: 16-byte granules)
                const half8* src = reinterpret_cast<const half8*>(wh + bd.dw + (size_t)ch0 * kk * kk);
                half8* dst = reinterpret_cast<half8*>(Pdw);
                for (int i = tid; i < (chunk * kk * kk) >> 3; i += 512) dst[i] = src[i];
            }
            const int tiles = (chunk >> 5) * 2, ct0 = ch0 >> 5;
            __syncthreads();                                            // parameters (and the ECA's x, or the gathered x) in place
            // phase 1 — 1x1 expand, transposed: Y1[ch][sq] = relu(W1^T x^T + b1)
            {
                const h16* brow = Xs + sqL * ldx + kh;
                for (int t = wave; t < tiles; t += 8) {
                    const int ct = t >> 1;
                    const floatx16 e = gemm_tile<true, NPF>(zero16(), brow, C >> 4, wh + bd.w1, copTiles, ct0 + ct, lane);
#pragma unroll
                    for (int rg = 0; rg < 16; ++rg) {
                        const int ch = ct * 32 + drow(rg, lane);
                        Y1[ch * 66 + sqL] = (h16)fmaxf(e[rg] + sb1[ch], 0.0f);
                    }
                }
            }
            __syncthreads();
            // phase 2 — depthwise kxk (+bias, ReLU) into Y2[sq][ch]
            for (int item = tid; item < chunk * 4; item += 512) {
                const int ch = item % chunk, g = item / chunk;
                const h16* wd = Pdw + (size_t)ch * kk * kk;
                if (!K5 || kk == 3) depthwise_rows_ld<3>(Y1 + ch * 66, Y2, ld2, ch, g, wd, sb2[ch]);
                else depthwise_rows_ld<5>(Y1 + ch * 66, Y2, ld2, ch, g, wd, sb2[ch]);
            }
            __syncthreads();
            // the chunk goes to columns [ch0, ch0 + chunk) of the team's Y region (the next chunk's depthwise phase — the next writer of
            // Y2 — starts behind the barrier after its expand phase)
            publish_cols(Y2, ld2, 0, tc.ry, cop, ch0, chunk, tid);
        }
        if (!team_sync<T>(tc)) return false;
        // phase 3 — 1x1 project of the member's C/T output channels over ALL expanded channels, k ascending; the chunks of Y2 alternate
        // between two LDS buffers, so one barrier per chunk is enough: a buffer is rewritten two chunks later, behind the barrier of the
        // chunk in between, which every wave passes after its MFMAs on that buffer
        floatx16 pacc[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) pacc[i] = zero16();
        for (int k0 = 0, it = 0; k0 < cop; k0 += CM, ++it) {
            const int pc = min(CM, cop - k0), ldb = pc + 8;
            h16* buf = U + (size_t)(it & 1) * 64 * (CM + 8);
            fetch_cols(buf, ldb, 0, tc.ry, cop, k0, pc, tid);
            __syncthreads();
            const h16* w2c = wh + bd.w2 + (size_t)(k0 >> 4) * ctiles * 512;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int lt = wave + 8 * i;
                if (lt < 2 * MT) pacc[i] = gemm_tile<false, NPF>(pacc[i], buf + sqL * ldb + kh, pc >> 4, w2c, ctiles, cbase + (lt >> 1), lane);
            }
        }
        // + bias + residual on the member's channels
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int lt = wave + 8 * i;
            if (lt < 2 * MT) {
                const int co = (cbase + (lt >> 1)) * 32 + (lane & 31);
                const float bias = sb3[co];
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    const int sq = stile * 32 + drow(rg, lane);
                    Xs[sq * ldx + co] = (h16)((float)Xs[sq * ldx + co] + pacc[i][rg] + bias);
                }
            }
        }
        __syncthreads();
        publish_cols(Xs, ldx, c0, tc.rx, C, c0, CW, tid);
        if (!team_sync<T>(tc)) return false;
        fetch_cols(Xs, ldx, 0, tc.rx, C, 0, c0, tid);
        fetch_cols(Xs, ldx, c0 + CW, tc.rx, C, c0 + CW, C - c0 - CW, tid);
        __syncthreads();
    }
    // ---- value head (member 0): 1x1 conv C -> cv (+bias, ReLU), NCHW flatten, linear -> (wdl x3, plys)
    if (m == 0) {
        const int cv = nd.cv;
        if (wave < 2) {
            const floatx16 e = gemm_tile<true, NPF>(zero16(), Xs + sqL * ldx + kh, C >> 4, wh + nd.v_w, 1, 0, lane);
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) {
                const int ch = drow(rg, lane);
                if (ch < cv) Y1[ch * 66 + sqL] = (h16)fmaxf(e[rg] + wf[nd.v_b + ch], 0.0f);
            }
        }
        __syncthreads();
        float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const h16* wl = wh + nd.vl_w;
        for (int i = tid; i < cv * 64; i += 512) {
            const float v = (float)Y1[(i >> 6) * 66 + (i & 63)];
#pragma unroll
            for (int o = 0; o < 4; ++o) part[o] += v * (float)wl[(size_t)o * cv * 64 + i];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float v = part[o];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) Ev[wave * 4 + o] = v;
        }
        __syncthreads();
        if (tid == 0) {
            float lo[4];
            for (int o = 0; o < 4; ++o) {
                float v = wf[nd.vl_b + o];
                for (int w8 = 0; w8 < 8; ++w8) v += Ev[w8 * 4 + o];
                lo[o] = v;
            }
            const float mx = fmaxf(lo[0], fmaxf(lo[1], lo[2]));
            const float e0 = __expf(lo[0] - mx), e1 = __expf(lo[1] - mx), e2 = __expf(lo[2] - mx);
            const float inv = 1.0f / (e0 + e1 + e2);
            value[sIdx] = (h16)((e2 - e0) * inv);
            wdl[sIdx * 3 + 0] = (h16)lo[0]; wdl[sIdx * 3 + 1] = (h16)lo[1]; wdl[sIdx * 3 + 2] = (h16)lo[2];
            ml[sIdx] = (h16)(1.0f / (1.0f + __expf(-lo[3])));
        }
        __syncthreads();                                                 // Y1 (inside U) is about to be overwritten by Ss
    }
    // ---- policy trunk: shared 3x3 conv C -> C (+bias, ReLU) into Ss, the member's channels; slices through the Y region
    for (int i = tid; i < ldx; i += 512) Ss[64 * ldx + i] = (h16)0.0f;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int lt = wave + 8 * i;
        if (lt < 2 * MT) {
            const int ctile = cbase + (lt >> 1);
            const floatx16 acc = gemm_conv3<ctiles * 2, false>(zero16(), Xs, sqL, ldx, 64, kh, wh + nd.ps_w, ctiles, ctile, lane);
            const int co = ctile * 32 + (lane & 31);
            const float bias = wf[nd.ps_b + co];
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) Ss[(stile * 32 + drow(rg, lane)) * ldx + co] = (h16)fmaxf(acc[rg] + bias, 0.0f);
        }
    }
    __syncthreads();
    publish_cols(Ss, ldx, c0, tc.ry, C, c0, CW, tid);
    if (!team_sync<T>(tc)) return false;
    fetch_cols(Ss, ldx, 0, tc.ry, C, 0, c0, tid);
    fetch_cols(Ss, ldx, c0 + CW, tc.ry, C, c0 + CW, C - c0 - CW, tid);
    __syncthreads();
    // ---- policy projection: 3x3 C -> 146 planes padded to 160 = 5 channel tiles x 2 square halves; tiles [m*10/T, (m+1)*10/T), one per wave
    {
        const int t = m * 10 / T + wave;
        if (t < (m + 1) * 10 / T) {
            const int ct = t >> 1, sq = (t & 1) * 32 + (lane & 31);
            const floatx16 e = gemm_conv3<ctiles * 2, true>(zero16(), Ss, sq, ldx, 64, kh, wh + nd.pp_w, 5, ct, lane);
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) {
                const int ch = ct * 32 + drow(rg, lane);
                if (ch < 73) piA[sIdx * HM_POLICY_VALUES + ch * 64 + sq] = (h16)e[rg];
                else if (ch < 146) piB[sIdx * HM_POLICY_VALUES + (ch - 73) * 64 + sq] = (h16)e[rg];
            }
        }
    }
    __syncthreads();                                                     // Ss is overwritten by the next position's input staging
    return true;
}

}  // namespace hmn
