// hm_net_xboard_device.hpp — device side of the cross-board tail (hm_net_xboard.hip): everything CrossBoardRiseV3
// (src/architectures/rise_mobile_v3.py:242-412 of the reference) does after the RISEv3 trunk, for one position, by one workgroup of
// 8 waves, with every activation in LDS or registers.
//
// Work split.  The 2 x 64 board tokens are four token tiles of 32 (tt = board * 2 + square half), the 192 channels six channel tiles.
// Wave w owns token tile w & 3 and the channel tiles (w >> 2) + 2i (i = 0, 1, 2) for the whole tail: its three fp32 residual tiles live
// in 48 accumulator registers per lane, in the transposed orientation (channels = MFMA rows, tokens = columns), so that the token
// projection writes them, the out-projection and mlp.2 accumulate straight onto them, and a token's LayerNorm sums are in-lane sums
// plus one cross-half shuffle and one LDS exchange with the partner wave w ^ 4.  A channel tile is a head (32 = head dimension), so the
// wave that owns residual tile (head, tt) also computes that head's Q tile and keeps it in registers as the score MFMA's operand.
//
// LayerNorm weights and biases are folded into the matrices that follow them on the host (Q, K, V, mlp.0), 1/sqrt(32) into Q, so one
// normalised fp16 copy of the tokens (XH) feeds Q, K and V alike.  Attention runs in three passes of two heads: K as [key][d] and V as
// [d][key] of those heads go to LDS (neither is computed twice), then each wave takes its (head, token tile): S^T = K Q^T with the keys
// down the registers (softmax = in-lane reduction + one shuffle), P stays in registers as the operand of O^T = V^T P.  The MFMA
// k index of both products is free to be permuted, and is: a lane's accumulator registers 8s .. 8s + 7 ARE its operand of k-step s
// (k slot 8h + j <-> row 16s + 4h + (j & 3) + 8(j >> 2), h = lane >> 5), and K / V are stored in that slot order.
//
// LDS (halfs):  XH [136][200]  normalised tokens (rows 0..127), normalised context tokens (128..134), a zero row (135); at the end
//                               the final tokens for the heads
//               OB [128][200]  attention output, then the MLP's hidden half; first the projection's input tile, last the value
//                               fusion map and the policy trunks (both run over into KP / VP, dead by then)
//               KP [136][72]   K of the pass's two heads: board tokens, context tokens, a zero row
//               VP [64][152]   V^T of the pass's two heads: 128 board keys + 16 context key slots (7 real, the rest zeros)
//               SC 2176 floats LayerNorm exchange, plane means, context tokens, head scratch
#pragma once
#include "hm_net_device.hpp"

namespace hmn {

constexpr int XB_D = 192, XB_LD = 200, XB_HEADS = 6, XB_KEYS = 71, XB_CTX = 7, XB_POL = 96;
constexpr int XB_XH = 136 * XB_LD, XB_OB = 128 * XB_LD, XB_KP = 136 * 72, XB_VP = 64 * 152, XB_SC = 2176;
constexpr size_t XB_LDS_BYTES = (size_t)(XB_XH + XB_OB + XB_KP + XB_VP) * 2 + XB_SC * 4;

struct XbLayer {
    unsigned wq, wk, wv, wo, w1, w2;     // fp16 offsets: packed [192][192] x4, [192][384], [384][192]
    unsigned bq, bk, bv, bo, b1, b2;     // fp32 offsets
};
struct XbDesc {
    int C, layers;
    float eps;
    int pad;
    unsigned tp_w[2], ph_w1[2], ph_w2[2], vf_w;                  // fp16: token projections [C + 48][192], policy 3x3s, value fusion [384][C]
    unsigned tp_b[2], ph_b1[2], vf_b;                            // fp32 biases (BatchNorm folded)
    unsigned pos_e, brd_e, pk_w, pk_b, sc_w, sc_b, role_e;       // fp32: embeddings [64][192], [2][192]; pocket [192][5] + [192]; scalar [192] + [192]; roles [7][192]
    XbLayer L[2];
};

__device__ __forceinline__ half8 pack8(const floatx16& a, int s) {
    half8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (h16)a[8 * s + j];
    return r;
}
// a transposed tile D[ch][tok] to a token-major fp16 tile: registers 4g .. 4g + 3 are channels 8g + 4h .. + 3 of this lane's token
__device__ __forceinline__ void store_tok(h16* row /* &T[tok][chTile * 32] */, const floatx16& a, int lane) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        half4v v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (h16)a[4 * g + r];
        *reinterpret_cast<half4v*>(row + 8 * g + 4 * (lane >> 5)) = v;
    }
}

// LayerNorm statistics of this wave's token column over all 192 channels (its own three tiles, the other row half by shuffle, the
// partner wave's three tiles through St), then the normalised values into XH.  Two passes: mean, then centred squares.
__device__ __forceinline__ void xb_layernorm(const floatx16 (&res)[3], float* St, h16* XH, float eps, int wave, int lane) {
    const int l = lane & 31;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s += res[i][r];
    }
    s += __shfl_xor(s, 32);
    if (lane < 32) St[wave * 32 + l] = s;
    __syncthreads();
    const float mean = (St[wave * 32 + l] + St[(wave ^ 4) * 32 + l]) * (1.0f / 192.0f);
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float d = res[i][r] - mean; q += d * d; }
    }
    q += __shfl_xor(q, 32);
    if (lane < 32) St[256 + wave * 32 + l] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf((St[256 + wave * 32 + l] + St[256 + (wave ^ 4) * 32 + l]) * (1.0f / 192.0f) + eps);
    h16* row = XH + ((wave & 3) * 32 + l) * XB_LD;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        floatx16 n;
#pragma unroll
        for (int r = 0; r < 16; ++r) n[r] = (res[i][r] - mean) * rstd;
        store_tok(row + ((wave >> 2) + 2 * i) * 32, n, lane);
    }
    __syncthreads();
}

// The tail of one position.  feat: [64][C] fp16 trunk features; pin: the position's input planes [74][64] fp16; outputs to row sIdx.
template <int CTILES>
__device__ __forceinline__ void xboard_position(const NetDesc& nd, const XbDesc& xd, const h16* __restrict__ wh, const float* __restrict__ wf,
                                                const h16* __restrict__ feat, const h16* __restrict__ pin, size_t sIdx, unsigned char* smem,
                                                h16* __restrict__ value, h16* __restrict__ piA, h16* __restrict__ piB, h16* __restrict__ wdl, h16* __restrict__ ml) {
    constexpr int C = CTILES * 32, ldin = C + 104, ldv = C + 8;
    h16* XH = reinterpret_cast<h16*>(smem);
    h16* OB = XH + XB_XH;
    h16* KP = OB + XB_OB;
    h16* VP = KP + XB_KP;
    float* St = reinterpret_cast<float*>(VP + XB_VP);            // [2][8][32] LayerNorm exchange
    float* Mn = St + 512;                                        // [23 x 8] partial sums, then [23] plane means at Mn + 192
    float* Ctx = Mn + 256;                                       // [7][192] context tokens, later the value head's scratch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 31, h = lane >> 5, kh = 8 * h;
    const int tt = wave & 3, board = tt >> 1, cw = wave >> 2;    // this wave's token tile, its board, its first channel tile
    const int tok = tt * 32 + l;                                 // this lane's token row in XH / OB
    const int sqb = (tt & 1) * 32 + l;                           // the same token as a square of its board

    // ---- stage the projection's input tile In[64][C | board A's 37 planes, zeros to 48 | board B's, zeros to 48] over OB..
    h16* In = OB;
    for (int i = tid; i < 64 * (C >> 3); i += 512) {
        const int sq = i / (C >> 3), c8 = i - sq * (C >> 3);
        *reinterpret_cast<frag4*>(In + sq * ldin + 8 * c8) = *reinterpret_cast<const frag4*>(feat + (size_t)sq * C + 8 * c8);
    }
    for (int i = tid; i < 64 * 96; i += 512) {
        const int sq = i & 63, col = i >> 6, b = col >= 48 ? 1 : 0, p = col - 48 * b;
        In[sq * ldin + C + col] = p < 37 ? pin[(37 * b + p) * 64 + sq] : (h16)0.0f;
    }
    for (int i = tid; i < XB_LD; i += 512) XH[135 * XB_LD + i] = (h16)0.0f;
    // plane means for the context tokens: pockets (planes 12..16, 17..21 of either board), plane 25 of either board, plane 31 of board A
    if (tid < 23 * 8) {
        const int it = tid >> 3, part = tid & 7;
        const int plane = it < 20 ? 37 * (it / 10) + 12 + it % 10 : it == 20 ? 25 : it == 21 ? 62 : 31;
        const half8 v = *reinterpret_cast<const half8*>(pin + plane * 64 + 8 * part);
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += (float)v[j];
        Mn[tid] = s;
    }
    __syncthreads();
    if (tid < 23) {
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += Mn[tid * 8 + j];
        Mn[192 + tid] = s * (1.0f / 64.0f);
    }
    // ---- token projections (1x1 over C + 37 channels, BatchNorm folded, ReLU) + position and board embeddings -> residual tiles
    floatx16 res[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ct = cw + 2 * i;
        const h16* w = wh + xd.tp_w[board];
        floatx16 a = gemm_tile<true, 8>(zero16(), In + sqb * ldin + kh, C >> 4, w, 6, ct, lane);
        a = gemm_tile<true, 3>(a, In + sqb * ldin + C + 48 * board + kh, 3, w + (size_t)(C >> 4) * 6 * 512, 6, ct, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = ct * 32 + drow(r, lane);
            res[i][r] = fmaxf(a[r] + wf[xd.tp_b[board] + ch], 0.0f) + wf[xd.pos_e + sqb * XB_D + ch] + wf[xd.brd_e + board * XB_D + ch];
        }
    }
    __syncthreads();                                             // In is dead; the plane means are there
    for (int i = tid; i < 72; i += 512) KP[135 * 72 + i] = (h16)0.0f;
    for (int i = tid; i < XB_CTX * XB_D; i += 512) {
        const int j = i / XB_D, c = i - j * XB_D;
        float v;
        if (j < 4) {
            v = wf[xd.pk_b + c];
#pragma unroll
            for (int k = 0; k < 5; ++k) v += wf[xd.pk_w + c * 5 + k] * Mn[192 + 5 * j + k];
        } else {
            v = wf[xd.sc_w + c] * Mn[192 + 16 + j] + wf[xd.sc_b + c];
        }
        Ctx[i] = v + wf[xd.role_e + i];
    }
    __syncthreads();
    if (wave < XB_CTX) {                                         // normalised context tokens (memory_norm's weight and bias are folded into K / V)
        const float x0 = Ctx[wave * XB_D + lane], x1 = Ctx[wave * XB_D + 64 + lane], x2 = Ctx[wave * XB_D + 128 + lane];
        float s = x0 + x1 + x2;
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        const float mean = s * (1.0f / 192.0f);
        const float d0 = x0 - mean, d1 = x1 - mean, d2 = x2 - mean;
        float q = d0 * d0 + d1 * d1 + d2 * d2;
        for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
        const float rstd = 1.0f / sqrtf(q * (1.0f / 192.0f) + xd.eps);
        h16* row = XH + (128 + wave) * XB_LD;
        row[lane] = (h16)(d0 * rstd); row[64 + lane] = (h16)(d1 * rstd); row[128 + lane] = (h16)(d2 * rstd);
    }

    for (int li = 0; li < xd.layers; ++li) {
        const XbLayer L = xd.L[li];
        xb_layernorm(res, St, XH, xd.eps, wave, lane);
        const h16* xrow = XH + tok * XB_LD + kh;
        // ---- cross attention, two heads per pass
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int head = cw + 2 * p;
            half8 qf[2];
            {
                floatx16 a = gemm_tile<true, 12>(zero16(), xrow, 12, wh + L.wq, 6, head, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) a[r] += wf[L.bq + head * 32 + drow(r, lane)];
                qf[0] = pack8(a, 0); qf[1] = pack8(a, 1);
            }
            for (int t = wave; t < 20; t += 8) {                 // K and V of heads 2p, 2p + 1: (kind, head, token tile incl. the context tile)
                const int kind = t / 10, rem = t - 10 * kind, hl = rem / 5, t5 = rem - 5 * hl;
                const int row = t5 < 4 ? t5 * 32 + l : (l < XB_CTX ? 128 + l : 135);
                const h16* xr = XH + row * XB_LD + kh;
                if (kind == 0) {                                 // K^T tile D[d][key]: registers 8s .. 8s + 7 -> slots 16s + 8h ..
                    floatx16 a = gemm_tile<true, 12>(zero16(), xr, 12, wh + L.wk, 6, 2 * p + hl, lane);
#pragma unroll
                    for (int r = 0; r < 16; ++r) a[r] += wf[L.bk + (2 * p + hl) * 32 + drow(r, lane)];
                    if (t5 < 4 || l < XB_CTX) {
                        h16* dst = KP + row * 72 + hl * 32 + kh;
                        *reinterpret_cast<half8*>(dst) = pack8(a, 0);
                        *reinterpret_cast<half8*>(dst + 16) = pack8(a, 1);
                    }
                } else {                                         // V tile D[key][d]: this lane's channel, keys down the registers
                    floatx16 a = gemm_tile<false, 12>(zero16(), xr, 12, wh + L.wv, 6, 2 * p + hl, lane);
                    const float bias = wf[L.bv + (2 * p + hl) * 32 + l];
                    h16* dst = VP + (hl * 32 + l) * 152 + t5 * 32 + kh;
                    if (t5 < 4) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) a[r] += bias;
                        *reinterpret_cast<half8*>(dst) = pack8(a, 0);
                        *reinterpret_cast<half8*>(dst + 16) = pack8(a, 1);
                    } else {                                     // context keys: one k-step of 16 slots, the padded ones finite zeros
                        half8 v;
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = (j & 3) + 8 * (j >> 2) + 4 * h < XB_CTX ? (h16)(a[j] + bias) : (h16)0.0f;
                        *reinterpret_cast<half8*>(dst) = v;
                    }
                }
            }
            __syncthreads();
            {   // this wave's (head, token tile): scores against the other board's 64 tokens and the 7 context tokens
                const int ob = 1 - board, hl = cw;
                floatx16 sc[3];
#pragma unroll
                for (int kt = 0; kt < 3; ++kt) {
                    const int row = kt < 2 ? ob * 64 + kt * 32 + l : (l < XB_CTX ? 128 + l : 135);
                    const h16* kr = KP + row * 72 + hl * 32 + kh;
                    sc[kt] = mfma(*reinterpret_cast<const half8*>(kr), qf[0], zero16());
                    sc[kt] = mfma(*reinterpret_cast<const half8*>(kr + 16), qf[1], sc[kt]);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) if (drow(r, lane) >= XB_CTX) sc[2][r] = -INFINITY;
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[kt][r]);
                }
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                float sum = 0.0f;
#pragma unroll
                for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) { sc[kt][r] = __expf(sc[kt][r] - mx); sum += sc[kt][r]; }
                }
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) sc[kt][r] *= inv;
                }
                floatx16 o = zero16();
                const h16* vr = VP + (hl * 32 + l) * 152 + kh;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    o = mfma(*reinterpret_cast<const half8*>(vr + ob * 64 + kt * 32), pack8(sc[kt], 0), o);
                    o = mfma(*reinterpret_cast<const half8*>(vr + ob * 64 + kt * 32 + 16), pack8(sc[kt], 1), o);
                }
                o = mfma(*reinterpret_cast<const half8*>(vr + 128), pack8(sc[2], 0), o);
                store_tok(OB + tok * XB_LD + head * 32, o, lane);
            }
            __syncthreads();
        }
        // ---- out-projection straight onto the residual
        const h16* orow = OB + tok * XB_LD + kh;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int ct = cw + 2 * i;
            res[i] = gemm_tile<true, 12>(res[i], orow, 12, wh + L.wo, 6, ct, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) res[i][r] += wf[L.bo + ct * 32 + drow(r, lane)];
        }
        // ---- MLP 192 -> 384 (exact GELU) -> 192 in two halves of the hidden channels, mlp.2 accumulating onto the residual
        xb_layernorm(res, St, XH, xd.eps, wave, lane);               // (its barriers also end the out-projection's reads of OB)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int ct = cw + 2 * i;
                floatx16 a = gemm_tile<true, 12>(zero16(), xrow, 12, wh + L.w1, 12, hh * 6 + ct, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float x = a[r] + wf[L.b1 + (hh * 6 + ct) * 32 + drow(r, lane)];
                    a[r] = 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
                }
                store_tok(OB + tok * XB_LD + ct * 32, a, lane);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 3; ++i)
                res[i] = gemm_tile<true, 12>(res[i], orow, 12, wh + L.w2 + (size_t)hh * 12 * 6 * 512, 6, cw + 2 * i, lane);
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) res[i][r] += wf[L.b2 + (cw + 2 * i) * 32 + drow(r, lane)];
        }
    }
    // ---- final board maps as fp16 tokens in XH (rows 0..63 board A, 64..127 board B; row 135 is still the zero row)
#pragma unroll
    for (int i = 0; i < 3; ++i) store_tok(XH + tok * XB_LD + (cw + 2 * i) * 32, res[i], lane);
    __syncthreads();
    // ---- value fusion: 1x1 over the concatenation (A, B), 384 -> C (+bias, ReLU) -> Vf[64][C + 8] over OB..
    h16* Vf = OB;
    {
        const int sq = (wave & 1) * 32 + l;
        for (int t = wave; t < 2 * CTILES; t += 8) {             // (t & 1) == (wave & 1): the tile's square half
            const int ct = t >> 1;
            floatx16 a = gemm_tile<true, 12>(zero16(), XH + sq * XB_LD + kh, 12, wh + xd.vf_w, CTILES, ct, lane);
            a = gemm_tile<true, 12>(a, XH + (64 + sq) * XB_LD + kh, 12, wh + xd.vf_w + (size_t)12 * CTILES * 512, CTILES, ct, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = fmaxf(a[r] + wf[xd.vf_b + ct * 32 + drow(r, lane)], 0.0f);
            store_tok(Vf + sq * ldv + ct * 32, a, lane);
        }
    }
    __syncthreads();
    // ---- value head on the fused map: the arithmetic of narrow_position (1x1 C -> cv, ReLU, NCHW flatten, 4 linear outputs)
    {
        h16* Y1 = OB + 64 * ldv;                                 // [cv][66]
        float* Ev = Ctx;
        const int cv = nd.cv;
        if (wave < 2) {
            const int sq = wave * 32 + l;
            const floatx16 e = gemm_tile<true, 8>(zero16(), Vf + sq * ldv + kh, C >> 4, wh + nd.v_w, 1, 0, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = drow(r, lane);
                if (ch < cv) Y1[ch * 66 + sq] = (h16)fmaxf(e[r] + wf[nd.v_b + ch], 0.0f);
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
        __syncthreads();                                         // Vf / Y1 are about to be overwritten by the policy trunks
    }
    // ---- policy heads, one per board, on the post-attention maps: 3x3 192 -> 192 (+bias, ReLU) -> P1[board][65][200], 3x3 192 -> 73
    h16* P1 = OB;
    for (int i = tid; i < 2 * XB_LD; i += 512) P1[((i >= XB_LD ? 65 : 0) + 64) * XB_LD + (i >= XB_LD ? i - XB_LD : i)] = (h16)0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ct = cw + 2 * i;
        floatx16 a = gemm_conv3<12, true>(zero16(), XH + board * 64 * XB_LD, sqb, XB_LD, 135 - 64 * board, kh, wh + xd.ph_w1[board], 6, ct, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = fmaxf(a[r] + wf[xd.ph_b1[board] + ct * 32 + drow(r, lane)], 0.0f);
        store_tok(P1 + (board * 65 + sqb) * XB_LD + ct * 32, a, lane);
    }
    __syncthreads();
    for (int t = wave; t < 12; t += 8) {                         // per board 73 planes padded to 96: 3 plane tiles x 2 square halves
        const int b = t / 6, rem = t - 6 * b, ct = rem >> 1, sq = (rem & 1) * 32 + l;
        const floatx16 e = gemm_conv3<12, true>(zero16(), P1 + b * 65 * XB_LD, sq, XB_LD, 64, kh, wh + xd.ph_w2[b], 3, ct, lane);
        h16* pi = (b ? piB : piA) + sIdx * HM_POLICY_VALUES;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int pl = ct * 32 + drow(r, lane);
            if (pl < 73) pi[pl * 64 + sq] = (h16)e[r];
        }
    }
    __syncthreads();                                             // the next position of this workgroup restages OB
}

}  // namespace hmn
