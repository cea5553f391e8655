// hm_net_pair_device.hpp — device side of the pair form of the fused RISEv3 forward (hm_net_pair.hip): TWO positions per workgroup of
// four waves, so that every weight fragment a wave fetches multiplies M = 128 rows (position 0 / 1 x square half 0 / 1) and feeds four
// independent MFMA chains.  Narrow trunks only (C = 64 or 128, one channel tile per wave).  Built on the fragment helpers of
// hm_net_device.hpp; per output element the k-step order, and the grouping of every reduction, are those of narrow_position4, so a
// row's results are bit-identical to the one-position forms and do not depend on the row it is paired with.
#pragma once
#include "hm_net_device.hpp"

namespace hmn {

// The four-accumulator counterparts of gemm_tile2_q / expand_stream2_q / gemm_conv3_2.  x[2 * p + h] is the LDS row pointer of this
// lane for position p, square half h; acc[2 * p + h] its accumulator.  The four MFMAs of a k-step are independent of one another.
template <bool WA>
__device__ __forceinline__ void mfma4(floatx16 (&acc)[4], const frag4 f, const frag4 (&x)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = WA ? mfma(h8(f), h8(x[a]), acc[a]) : mfma(h8(x[a]), h8(f), acc[a]);
}
// continues from a queue fragq_fill has requested for the same (w, ntiles, tile, ksteps)
template <bool WA, int Q>
__device__ __forceinline__ void gemm_tile4_q(FragQ<Q>& f, floatx16 (&acc)[4], const h16* const (&xr)[4], int ksteps, const h16* w, int ntiles, int tile, int lane) {
    const frag4* wp = reinterpret_cast<const frag4*>(w) + (size_t)tile * 64 + lane;
    const size_t ws = (size_t)ntiles * 64;
    const int last = ksteps - 1;
    int base = 0;
    for (; base + Q < ksteps; base += Q) {
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            frag4 x[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) x[a] = lds_frag(xr[a] + (base + j) * 16);
            const frag4 fr = f.q[j];
            const int nxt = base + Q + j;
            f.q[j] = wp[(size_t)(nxt < last ? nxt : last) * ws];
            mfma4<WA>(acc, fr, x);
        }
    }
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        if (base + j < ksteps) {
            frag4 x[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) x[a] = lds_frag(xr[a] + (base + j) * 16);
            mfma4<WA>(acc, f.q[j], x);
        }
    }
}
template <bool WA, int Q>
__device__ __forceinline__ void gemm_tile4(floatx16 (&acc)[4], const h16* const (&xr)[4], int ksteps, const h16* w, int ntiles, int tile, int lane) {
    FragQ<Q> f;
    fragq_fill<Q>(f, w, ntiles, tile, ksteps, lane);
    gemm_tile4_q<WA, Q>(f, acc, xr, ksteps, w, ntiles, tile, lane);
}
// A wave's tiles of the transposed expand GEMM as one fragment stream (expand_stream2_q: ksteps == Q, queue requested by fragq_fill for
// the first tile); epi(i, acc) stores the four 32x32 results of tile i.
template <int Q, typename Epi>
__device__ __forceinline__ void expand_stream4_q(FragQ<Q>& f, const h16* const (&xr)[4], int ksteps, const h16* w, int ntiles, int tile0, int tstride, int ntile, int lane, Epi&& epi) {
    const frag4* base = reinterpret_cast<const frag4*>(w) + lane;
    const size_t ws = (size_t)ntiles * 64;
    const frag4* wp = base + (size_t)tile0 * 64;
    for (int i = 0; i < ntile; ++i) {
        const frag4* wn = base + (size_t)(tile0 + (i + 1 < ntile ? i + 1 : i) * tstride) * 64;
        floatx16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
        for (int b = 0; b < ksteps; b += Q) {
            const frag4* nx = b + Q < ksteps ? wp + (size_t)(b + Q) * ws : wn;
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                frag4 x[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) x[a] = lds_frag(xr[a] + (b + j) * 16);
                const frag4 fr = f.q[j];
                f.q[j] = nx[(size_t)j * ws];
                mfma4<true>(acc, fr, x);
            }
        }
        epi(i, acc);
        wp = wn;
    }
}
// 3x3 convolution (gemm_conv3_2) for both positions: `act` is position 0's tile, position 1's lies pstride halfs behind it
template <int KPT, bool WA>
__device__ __forceinline__ void gemm_conv3_4(floatx16 (&acc)[4], const h16* act, int pstride, int sq0, int pitch, int zeroRow, int kh, const h16* w, int ntiles, int tile, int lane) {
    const frag4* wp = reinterpret_cast<const frag4*>(w) + (size_t)tile * 64 + lane;
    const size_t ws = (size_t)ntiles * 64;
    frag4 q[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) q[j] = wp[(size_t)j * ws];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const h16* ap0 = act + im2col_row(sq0, t, pitch, zeroRow) + kh;
        const h16* ap1 = act + im2col_row(sq0 + 32, t, pitch, zeroRow) + kh;
#pragma unroll
        for (int kk = 0; kk < KPT; ++kk) {
            const frag4 x[4] = {lds_frag(ap0 + kk * 16), lds_frag(ap1 + kk * 16), lds_frag(ap0 + pstride + kk * 16), lds_frag(ap1 + pstride + kk * 16)};
            const frag4 f = q[kk];
            if (t < 8) q[kk] = wp[(size_t)((t + 1) * KPT + kk) * ws];
            mfma4<WA>(acc, f, x);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

#define HM_STAMP() do { if (dbg && blockIdx.x == 0 && threadIdx.x == 0 && dbgN < 256) dbg[dbgN++] = __builtin_amdgcn_s_memtime(); } while (0)

// Two positions through the whole network by one workgroup of four waves.  pin[p]: input planes of position p; row[p]: its row of the
// head tensors; st[p]: whether its heads are stored (a dead partner is computed on the live row's planes and stores nothing).
// LDS: Xs[2][65][C+8] | union per position { Ss[65][C+8] , Y1[copMax][66] + Y2[64][copMax+8] } x 2 (uPos halfs each) | per-chunk
// parameters b1, b2, b3, depthwise taps (staged once for both positions) | ECA / head scratch x 2.
template <int CTILES, bool K5>
__device__ __forceinline__ void pair_position(const NetDesc& nd, const h16* __restrict__ wh, const float* __restrict__ wf, const h16* const (&pin)[2],
                                              const size_t (&row)[2], const bool (&st)[2], int copMax, int uPos, unsigned char* smem,
                                              h16* __restrict__ value, h16* __restrict__ piA, h16* __restrict__ piB, h16* __restrict__ wdl, h16* __restrict__ ml,
                                              unsigned long long* __restrict__ dbg, int& dbgN) {
    static_assert(CTILES == 2 || CTILES == 4, "pair form: C = 64 or 128 (one channel tile per wave)");
    constexpr int C = CTILES * 32, ldx = C + 8, ctiles = CTILES, NPF = 8, XP = 65 * ldx, EVP = 5 * C + 64;
    constexpr bool PF = HM_NET_PREFETCH != 0;
    h16* Xs = reinterpret_cast<h16*>(smem);                             // [2][65][ldx]
    h16* U = Xs + 2 * XP;                                               // union region: position p at U + p * uPos
    h16* Ss = U;                                                        // [65][ldx] (input staging uses pitch ldi)
    h16* Y1 = U;                                                        // [chunk][66]
    h16* Y2 = U + (size_t)copMax * 66;                                  // [64][chunk + 8]
    float* Pf = reinterpret_cast<float*>(U + 2 * (size_t)uPos);         // b1[chunk], b2[chunk], b3[C]  (uPos % 8 == 0)
    h16* Pdw = reinterpret_cast<h16*>(Pf + 2 * copMax + C);             // depthwise weights [chunk][k*k]
    float* Ev = reinterpret_cast<float*>(Pdw + (((size_t)copMax * 25 + 7) & ~(size_t)7));   // per position: [4][C] + [C] + 64
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = 8 * (lane >> 5);
    const int sq0 = lane & 31;
    const bool own = wave < ctiles;                                     // this wave's channel tile of an N = C GEMM is `wave`

    HM_STAMP();
    // ---- input planes: NCHW [74][64] fp16 -> Ss as [sq][cin_pad] (+ zero row 64), both positions
    const int ldi = nd.cin_pad + 8;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const frag4 z = {0, 0, 0, 0};
        frag4* z16 = reinterpret_cast<frag4*>(Ss + p * uPos);
        for (int i = tid; i < (65 * ldi) >> 3; i += 256) z16[i] = z;
        for (int i = tid; i < ldx; i += 256) Xs[p * XP + 64 * ldx + i] = (h16)0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        h16* S = Ss + p * uPos;
        for (int c = tid; c < HM_PLANE_VALUES / 8; c += 256) {
            const half8 v = *reinterpret_cast<const half8*>(pin[p] + 8 * c);
            const int pl = c >> 3, sq8 = (c & 7) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) S[(sq8 + j) * ldi + pl] = v[j];
        }
    }
    __syncthreads();
    HM_STAMP();   // input staged
    // ---- stem: 3x3 conv cin -> C (+bias, ReLU)
    if (own) {
        floatx16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
        gemm_conv3_4<5, false>(acc, Ss, uPos, sq0, ldi, 64, kh, wh + nd.stem_w, ctiles, wave, lane);
        const int co = wave * 32 + (lane & 31);
        const float bias = wf[nd.stem_b + co];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            h16* X = Xs + (a >> 1) * XP + (a & 1) * 32 * ldx;
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) X[drow(rg, lane) * ldx + co] = (h16)fmaxf(acc[a][rg] + bias, 0.0f);
        }
    }
    // the expand GEMM's first weight fragments are requested one phase ahead (FragQ), as in narrow_position4; a wave that has no tile
    // of the coming chunk requests the chunk's last one (its queue is not used), so that no request leaves the matrix
    FragQ<NPF> eq;
    if (PF && nd.nblocks > 0) fragq_fill<NPF>(eq, wh + nd.blk[0].w1, nd.blk[0].cop >> 5, min(wave, (nd.blk[0].cop >> 5) - 1), C >> 4, lane);
    __syncthreads();
    HM_STAMP();
    // ---- mobile bottleneck blocks
    for (int bi = 0; bi < nd.nblocks; ++bi) {
        const BlockDesc bd = nd.blk[bi];
        const int cop = bd.cop, kk = bd.k;
        float* sb1 = Pf; float* sb2 = Pf + copMax; float* sb3 = Pf + 2 * copMax;
        for (int i = tid; i < C; i += 256) sb3[i] = wf[bd.b3 + i];
        if (bd.eca) {   // x = x * hardsigmoid(W_eca . mean_sq(x) + b), grouped as narrow_position4 groups it
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float* part = Ev + p * EVP;
                const h16* X = Xs + p * XP;
                for (int it = tid; it < 4 * C; it += 256) {
                    const int c = it % C, q = it / C;
                    h16 xv[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) xv[j] = X[(16 * q + j) * ldx + c];
                    float sacc = 0.0f;
#pragma unroll
                    for (int j = 0; j < 16; ++j) sacc += (float)xv[j];
                    part[q * C + c] = sacc;
                }
            }
            __syncthreads();
            for (int i = tid; i < 2 * C; i += 256) {
                const int p = i / C, c = i - p * C;
                const float* part = Ev + p * EVP;
                Ev[p * EVP + 4 * C + c] = (part[c] + part[C + c] + part[2 * C + c] + part[3 * C + c]) * (1.0f / 64.0f);
            }
            __syncthreads();
            // W_eca . mean: work item = (1/32 of the input channels, 8 adjacent output channels); a thread's rows are fetched once and
            // multiply both positions' means.  The 32 partial sums per channel go through each position's union region.
            {
                const h16* we = wh + bd.ecaw;                           // [ci][co]
                constexpr int CG = C >> 3, ROWS = C >> 5;
                for (int it = tid; it < 32 * CG; it += 256) {
                    const int cg = it % CG, q = it / CG;
                    const h16* wrow = we + (size_t)(q * ROWS) * C + 8 * cg;
                    half8 w8[ROWS];
#pragma unroll
                    for (int u = 0; u < ROWS; ++u) w8[u] = *reinterpret_cast<const half8*>(wrow + (size_t)u * C);
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        const float* Mv = Ev + p * EVP + 4 * C;
                        float s[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int u = 0; u < ROWS; ++u) {
                            const float m = Mv[q * ROWS + u];
#pragma unroll
                            for (int k = 0; k < 8; ++k) s[k] += (float)w8[u][k] * m;
                        }
                        float* dst = reinterpret_cast<float*>(U + p * uPos) + q * C + 8 * cg;
#pragma unroll
                        for (int k = 0; k < 8; ++k) dst[k] = s[k];
                    }
                }
            }
            __syncthreads();
            for (int i = tid; i < 2 * C; i += 256) {
                const int p = i / C, c = i - p * C;
                const float* part32 = reinterpret_cast<const float*>(U + p * uPos);
                float sg = wf[bd.ecab + c];
#pragma unroll
                for (int q = 0; q < 32; ++q) sg += part32[q * C + c];
                Ev[p * EVP + 4 * C + c] = fminf(fmaxf(sg * (1.0f / 6.0f) + 0.5f, 0.0f), 1.0f);
            }
            __syncthreads();
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const float* Mv = Ev + p * EVP + 4 * C;
                h16* X = Xs + p * XP;
#pragma unroll 4
                for (int i = tid; i < 32 * C; i += 256) {               // two adjacent channels per item
                    const int sq = i / (C >> 1), cc = 2 * (i - sq * (C >> 1));
                    half2v* px = reinterpret_cast<half2v*>(X + sq * ldx + cc);
                    half2v x2 = *px;
                    x2[0] = (h16)((float)x2[0] * Mv[cc]); x2[1] = (h16)((float)x2[1] * Mv[cc + 1]);
                    *px = x2;
                }
            }
        }
        floatx16 pacc[4] = {zero16(), zero16(), zero16(), zero16()};   // projection accumulators (position, square half), carried over the chunks
        for (int ch0 = 0; ch0 < cop; ch0 += copMax) {
            const int chunk = min(copMax, cop - ch0), ld2 = chunk + 8;
            // parameter stage of this chunk, once for both positions
            {
                for (int i = tid; i < chunk; i += 256) { sb1[i] = wf[bd.b1 + ch0 + i]; sb2[i] = wf[bd.b2 + ch0 + i]; }
                const half8* src = reinterpret_cast<const half8*>(wh + bd.dw + (size_t)ch0 * kk * kk);
                half8* dst = reinterpret_cast<half8*>(Pdw);
                for (int i = tid; i < (chunk * kk * kk) >> 3; i += 256) dst[i] = src[i];
            }
            const int copTiles = cop >> 5, ct0 = ch0 >> 5, ctl = chunk >> 5;
            __syncthreads();
            HM_STAMP();   // parameters staged (+ ECA)
            // phase 1 — 1x1 expand, transposed: Y1[p][ch][sq] = relu(W1^T x^T + b1); the chunk's channel tiles over 4 waves
            {
                const h16* b0 = Xs + sq0 * ldx + kh;
                const h16* const xr[4] = {b0, b0 + 32 * ldx, b0 + XP, b0 + XP + 32 * ldx};
                auto store = [&](int ct, const floatx16 (&e)[4]) {
#pragma unroll
                    for (int rg = 0; rg < 16; ++rg) {
                        const int ch = ct * 32 + drow(rg, lane);
                        const float b = sb1[ch];
#pragma unroll
                        for (int a = 0; a < 4; ++a) Y1[(a >> 1) * uPos + ch * 66 + (a & 1) * 32 + sq0] = (h16)fmaxf(e[a][rg] + b, 0.0f);
                    }
                };
                if constexpr ((C >> 4) == NPF) {                        // C = 128: K = one queue, a wave's tiles as one fragment stream
                    const int ntile = ctl > wave ? (ctl - wave + 3) >> 2 : 0;
                    if (ntile > 0) {
                        if (!PF) fragq_fill<NPF>(eq, wh + bd.w1, copTiles, ct0 + wave, C >> 4, lane);
                        expand_stream4_q<NPF>(eq, xr, C >> 4, wh + bd.w1, copTiles, ct0 + wave, 4, ntile, lane,
                                              [&](int i, const floatx16 (&e)[4]) { store(wave + 4 * i, e); });
                    }
                } else {
                    for (int ct = wave; ct < ctl; ct += 4) {
                        floatx16 e[4] = {zero16(), zero16(), zero16(), zero16()};
                        if (PF && ct == wave) gemm_tile4_q<true, NPF>(eq, e, xr, C >> 4, wh + bd.w1, copTiles, ct0 + ct, lane);
                        else gemm_tile4<true, NPF>(e, xr, C >> 4, wh + bd.w1, copTiles, ct0 + ct, lane);
                        store(ct, e);
                    }
                }
            }
            __syncthreads();
            HM_STAMP();   // expand done
            // phase 2 — depthwise kxk (+bias, ReLU): work item = (channel, pair of board rows) for both positions, so that one
            // position's LDS reads overlap the other's arithmetic
            const h16* w2c = wh + bd.w2 + (size_t)(ch0 >> 4) * ctiles * 512;
            for (int item = tid; item < chunk * 4; item += 256) {
                const int ch = item % chunk, g = item / chunk;
                const float b2 = sb2[ch];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    if (!K5 || kk == 3) depthwise_rows_ld<3>(Y1 + p * uPos + ch * 66, Y2 + p * uPos, ld2, ch, g, Pdw + (size_t)ch * 9, b2);
                    else depthwise_rows_ld<5>(Y1 + p * uPos + ch * 66, Y2 + p * uPos, ld2, ch, g, Pdw + (size_t)ch * 25, b2);
                }
            }
            __syncthreads();
            HM_STAMP();   // depthwise done
            // phase 3 — 1x1 project, K = this chunk's channels: k-steps ch0/16 .. of W2
            if (own) {
                const h16* y0 = Y2 + sq0 * ld2 + kh;
                const h16* const yr[4] = {y0, y0 + 32 * ld2, y0 + uPos, y0 + uPos + 32 * ld2};
                gemm_tile4<false, NPF>(pacc, yr, chunk >> 4, w2c, ctiles, wave, lane);
            }
            if (PF) {   // the expand fragments of what comes next: this block's next chunk, or the next block's first one
                if (ch0 + copMax < cop) fragq_fill<NPF>(eq, wh + bd.w1, copTiles, min(((ch0 + copMax) >> 5) + wave, copTiles - 1), C >> 4, lane);
                else if (bi + 1 < nd.nblocks) fragq_fill<NPF>(eq, wh + nd.blk[bi + 1].w1, nd.blk[bi + 1].cop >> 5, min(wave, (nd.blk[bi + 1].cop >> 5) - 1), C >> 4, lane);
            }
            // (no barrier here: the next chunk's parameter stage and expand phase touch Pf / Pdw / Y1, which this phase does not read, and
            // its depthwise phase — the next writer of Y2 — starts behind the barrier after its expand phase)
        }
        // + bias + residual
        if (own) {
            const int co = wave * 32 + (lane & 31);
            const float bias = sb3[co];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                h16* X = Xs + (a >> 1) * XP + (a & 1) * 32 * ldx;
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    h16* px = X + drow(rg, lane) * ldx + co;
                    *px = (h16)((float)*px + pacc[a][rg] + bias);
                }
            }
        }
        __syncthreads();
        HM_STAMP();
    }
    // ---- value head: 1x1 conv C -> cv (+bias, ReLU), NCHW flatten, linear -> (wdl x3, plys)
    {
        const int cv = nd.cv;
        {   // one (position, square half) per wave
            const int p = wave >> 1, sqh = (wave & 1) * 32 + sq0;
            const floatx16 e = gemm_tile<true, NPF>(zero16(), Xs + p * XP + sqh * ldx + kh, C >> 4, wh + nd.v_w, 1, 0, lane);
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) {
                const int ch = drow(rg, lane);
                if (ch < cv) Y1[p * uPos + ch * 66 + sqh] = (h16)fmaxf(e[rg] + wf[nd.v_b + ch], 0.0f);
            }
        }
        __syncthreads();
        // partial sums grouped as narrow_position4 documents: each thread plays the threads t and t + 256 of the 8-wave form, a wave's 64
        // lanes are reduced together, the eight wave sums are added in order
        const h16* wl = wh + nd.vl_w;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int vh = 0; vh < 2; ++vh) {
                float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int i = tid + 256 * vh; i < cv * 64; i += 512) {
                    const float v = (float)Y1[p * uPos + (i >> 6) * 66 + (i & 63)];
#pragma unroll
                    for (int o = 0; o < 4; ++o) part[o] += v * (float)wl[(size_t)o * cv * 64 + i];
                }
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    float v = part[o];
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                    if (lane == 0) Ev[p * EVP + (wave + 4 * vh) * 4 + o] = v;
                }
            }
        }
        __syncthreads();
        if ((tid == 0 && st[0]) || (tid == 64 && st[1])) {             // one wave per position
            const int p = tid >> 6;
            const size_t sIdx = row[p];
            float lo[4];
            for (int o = 0; o < 4; ++o) {
                float v = wf[nd.vl_b + o];
                for (int w8 = 0; w8 < 8; ++w8) v += Ev[p * EVP + w8 * 4 + o];
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
    HM_STAMP();
    // ---- policy heads: shared 3x3 conv C -> C (+bias, ReLU) into Ss, then 3x3 C -> 146 (two boards)
    for (int i = tid; i < 2 * ldx; i += 256) Ss[(i / ldx) * uPos + 64 * ldx + i % ldx] = (h16)0.0f;
    if (own) {
        floatx16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
        gemm_conv3_4<CTILES * 2, false>(acc, Xs, XP, sq0, ldx, 64, kh, wh + nd.ps_w, ctiles, wave, lane);
        const int co = wave * 32 + (lane & 31);
        const float bias = wf[nd.ps_b + co];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            h16* S = Ss + (a >> 1) * uPos + (a & 1) * 32 * ldx;
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) S[drow(rg, lane) * ldx + co] = (h16)fmaxf(acc[a][rg] + bias, 0.0f);
        }
    }
    __syncthreads();
    HM_STAMP();
    {
        // 146 output planes padded to 160 = 5 channel tiles: tiles 0..3 on waves 0..3 for both positions and square halves, tile 4 as
        // four single tiles (position, square half), one per wave
        auto put = [&](int p, int ch, int sq, float v) {
            if (!st[p]) return;
            if (ch < 73) piA[row[p] * HM_POLICY_VALUES + ch * 64 + sq] = (h16)v;
            else if (ch < 146) piB[row[p] * HM_POLICY_VALUES + (ch - 73) * 64 + sq] = (h16)v;
        };
        {
            floatx16 e[4] = {zero16(), zero16(), zero16(), zero16()};
            gemm_conv3_4<CTILES * 2, true>(e, Ss, uPos, sq0, ldx, 64, kh, wh + nd.pp_w, 5, wave, lane);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) put(a >> 1, wave * 32 + drow(rg, lane), (a & 1) * 32 + sq0, e[a][rg]);
            }
        }
        {
            const int p = wave >> 1, sqh = (wave & 1) * 32 + sq0;
            const floatx16 e = gemm_conv3<CTILES * 2, true>(zero16(), Ss + p * uPos, sqh, ldx, 64, kh, wh + nd.pp_w, 5, 4, lane);
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) put(p, 4 * 32 + drow(rg, lane), sqh, e[rg]);
        }
    }
    __syncthreads();                                                     // the next pair's input staging overwrites Ss
    HM_STAMP();
}

#undef HM_STAMP

}  // namespace hmn
