// wavenet_forward.h -- k_wnf_*: the teacher-forced pass of the Gaussian WaveNet (Wavenet.forward, src/models/wavenet.py:83-91,
// src/models/modules.py:36-86) over all positions at once (gfx950).
//
// With x known nothing is sequential: every layer is a dense product over all positions.  The family puts TIME on the N side
// of v_mfma_f32_16x16x4_f32 and runs one launch per stage on the caller's stream -- a layer reads h(p - dil) from other time
// tiles, and the launch boundary is the only exchange between workgroups (no grid-wide barrier, no spinning, no residency
// assumption; the receptive field of 2 078 samples rules out fusing the layers over one tile with a halo):
//   k_wnf_inputs   x [B][N] -> the net's input channels [B][inp][N]: u(p) = x(p-1), exc(p-1), pred(p)      (plain HIP)
//   k_wnf_front    the 32-tap front convolution + ReLU -> h0 [B][R][N]
//   k_wnf_layer    one residual block: h_in -> h_out, skip += ...                          (one launch per block)
//   k_wnf_final    relu(skip + b_skip) -> S x S + ReLU -> 2 x S + b -> stats [B][N][2]
//
// Work split of the three MFMA kernels.  A workgroup of 16 wavefronts owns one utterance x one tile of TN (16, 32 or 64)
// consecutive positions, all channels.  A wavefront owns whole 16-row M tiles as in k_wn_decode, and runs the very same
// `gemm` loop on the very same packed weights (w_front, w1, w2, w_f1, w_f2 of fpc_wavenet_create: no second packing):
// every 16-byte A word now feeds TN / 16 N tiles from registers where the sample loop feeds one or two, which is the whole
// advantage -- the weight stream per position falls by TN / NU -- and the next word is still in flight while the MFMAs of
// the current one issue.
//
// k_wnf_layer, LDS map (floats; a panel is [rows][16], one per N tile, so the B read of a k-step is 64 consecutive floats):
//   BA  [TN/16][2R + coutp][16]  rows [0,R) h(p - dil), [R,2R) h(p), [2R,2R+coutp) c(p)
//   Z   [TN/16][G][16]           z = tanh(f) sigmoid(g)
// (2R + coutp + G) TN floats: 80 KiB at TN = 32 and 160 KiB at TN = 64 for R/G/S 128/256/128, cout 128.
// h(p - dil) comes from the previous stage's [B][R][N] buffer at the shifted offset, zeros where p - dil < 0 (each layer
// zero-pads its own input); positions past N are staged as zeros and never stored.
//   GEMM1 [2G x (2R + coutp)] . [(2R + coutp) x TN]: a wavefront carries the filter and the gate tile of the same 16
//         channels; gating in the accumulators -> Z.
//   GEMM2 [(R + S) x G] . [G x TN]: the R/16 residual tiles and the S/16 skip tiles are dealt round robin over the 16
//         wavefronts.  A residual tile writes (h + (acc + b_res)) sqrt(1/2) to h_out; a skip tile takes the running skip sum
//         from the skip buffer as the MFMA's C operand, adds this layer's K steps and stores it back.
//
// Numerics.  K ascends from zero in the sample loop's order, biases are added last, tanh_e / sigmoid_e, no packed fp32,
// columns never mix: every position's value runs through the same chain of instructions as in k_wn_decode with xin set, so
// the stats are bit-identical to the sequential fpc_wavenet_forward, whatever TN (tests).
#pragma once
#include "wavenet_decode.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace fpc_wn {

struct ForwardParams {
    int B, N, T, tiles;               // utterances, samples (160 T), frames, time tiles per utterance
    int R, G, S, cout, coutp, inp;
    int K0q, K1q, Gq, Sq;             // 16-wide K groups of the front layer, GEMM1, GEMM2, the last stage
    const float4* w_front;            // [R/16][K0q][64]
    const float* b_front;             // [R]
    const float4* w1;                 // [G/16][2][K1q][64]   of THIS layer
    const float* b1;                  // [2][G]
    const float4* w2;                 // [(R+S)/16][Gq][64]
    const float* b_res;               // [R]
    const float* b_skip;              // [S] summed over the layers
    const float4* w_f1;               // [S/16][Sq][64]
    const float* b_f1;                // [S]
    const float4* w_f2;               // [1][Sq][64]
    float b_f2[2];
    int dil, first, last;             // of this layer; first: the skip sum starts at zero; last: no residual output
    const float* x;                   // [B][N]        (k_wnf_inputs)
    const float* lpc;                 // [B][T][16]
    float* inp_out;                   // [B][inp][N]   (k_wnf_inputs writes)
    const float* inp_in;              // [B][inp][N]   (k_wnf_front reads)
    const float* cfeat;               // [B][cout][N]
    const float* hin;                 // [B][R][N]
    float* hout;                      // [B][R][N]
    float* skip;                      // [B][S][N]
    float* stats;                     // [B][N][2]
    float* ts;                        // [B][2G][N] of THIS layer: t = tanh(a_f), s = sigmoid(a_g)   (SAVE instances only)
    float* osave;                     // [B][S][N]: the last stage's hidden ReLU output              (SAVE instances only)
};

// The net's input at position p, as k_wn_decode's stage 0 and tail build it: u = x(p-1); with inp = 3 also
// exc(p-1) = x(p-1) - pred(p-1) and pred(p) = -sum_k a[frame(p)][k] x(p-1-k), the history before the utterance zero.
__global__ __launch_bounds__(256) void k_wnf_inputs(const ForwardParams p) {
    const long long N = p.N, total = (long long)p.B * N;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long b = idx / N;
        const int i = (int)(idx % N);
        const float* x = p.x + b * N;
        const auto pred_at = [&](int q) {
            const float* a = p.lpc + (b * p.T + q / 160) * 16;
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s = lpc_tap(s, a[k], q - 1 - k >= 0 ? x[q - 1 - k] : 0.0f);
            return -s;
        };
        float* o = p.inp_out + b * p.inp * N + i;
        const float u = i ? x[i - 1] : 0.0f;
        o[0] = u;
        if (p.inp == 3) {
            o[N] = i ? u - pred_at(i - 1) : 0.0f;
            o[2 * N] = pred_at(i);
        }
    }
}

// acc[nt] += A[16 x 16 KQ] . B, B(k, column) = Bp[off(k) + column]: `gemm` with a free B address per K index, for the
// Toeplitz read of the front convolution.  Same K order, same one-word lookahead.
template <int NT, class OffFn>
__device__ __forceinline__ void gemm_at(const float4* A, int KQ, const float* Bp, OffFn off, int lane, f32x4 (&acc)[NT]) {
    const int kl = lane >> 4, j = lane & 15;
    float4 cur = A[lane];
    for (int q = 0; q < KQ; ++q) {
        const float4 nxt = A[(q + 1 < KQ ? q + 1 : q) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* s = Bp + off(q * 16 + i * 4 + kl) + j;
            const float av = i == 0 ? cur.x : i == 1 ? cur.y : i == 2 ? cur.z : cur.w;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s[nt * 16], acc[nt], 0, 0, 0);
        }
        cur = nxt;
    }
}

// the workgroup's utterance and first position
__device__ __forceinline__ void tile_of_block(const ForwardParams& p, int TN, long long& b, int& p0) {
    b = blockIdx.x / p.tiles;
    p0 = (int)(blockIdx.x % p.tiles) * TN;
}

// Front convolution (wavenet.py:37-40): K index = channel * 32 + tap, tap k of a channel multiplies the input at position
// p - 31 + k.  LDS: XI [inp][TN + 32], the tile's inputs with a halo of 31 before it (zeros before the utterance).
template <int TN>
__global__ __launch_bounds__(THREADS) void k_wnf_front(const ForwardParams p) {
    constexpr int NT = TN / 16, W = TN + FRONT;
    extern __shared__ float lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kl = lane >> 4, j = lane & 15;
    const long long N = p.N;
    long long b;
    int p0;
    tile_of_block(p, TN, b, p0);
    for (int e = tid; e < p.inp * W; e += THREADS) {
        const int c = e / W;
        const long long pos = (long long)p0 - (FRONT - 1) + e % W;
        lds[e] = (pos >= 0 && pos < N) ? p.inp_in[(b * p.inp + c) * N + pos] : 0.0f;
    }
    __syncthreads();
    for (int t = wave; t < p.R / 16; t += WAVES) {
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 bias = bias_tile(p.b_front, t, lane);
        gemm_at<NT>(p.w_front + (long long)t * p.K0q * 64, p.K0q, lds, [](int k) { return (k >> 5) * W + (k & 31); }, lane, acc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long pos = p0 + nt * 16 + j;
                if (pos < N) p.hout[(b * p.R + t * 16 + 4 * kl + r) * N + pos] = fmaxf(acc[nt][r] + bias[r], 0.0f);
            }
    }
}

// rows [row0, row0 + nrows) of the panels at `dst` (panel stride ps) <- src[row][p - shift] of the tile's positions, in LDS
// order; zeros for rows >= src_rows, positions >= N and p - shift < 0
__device__ __forceinline__ void stage_rows(float* dst, int ps, int row0, int nrows, int nt_count, const float* src, int src_rows,
                                           long long N, int p0, int shift, int tid) {
    const int per = nrows * 16;
#pragma unroll 4
    for (int l = tid; l < nt_count * per; l += THREADS) {
        const int nt = l / per, rem = l - nt * per, row = rem >> 4, j = rem & 15;
        const long long pos = (long long)p0 + nt * 16 + j, q = pos - shift;
        const bool ok = row < src_rows && pos < N && q >= 0;
        const float v = ok ? src[row * N + q] : 0.0f;
        dst[nt * ps + (row0 + row) * 16 + j] = v;
    }
}

// One residual block (modules.py:62-77) for one utterance x TN positions.  SAVE (wavenet_backward.h): t and s also go to
// p.ts for the backward pass; the arithmetic is the same, so the stats are the same bits.
template <int TN, bool SAVE = false>
__global__ __launch_bounds__(THREADS) void k_wnf_layer(const ForwardParams p) {
    constexpr int NT = TN / 16;
    extern __shared__ float lds[];
    const int R = p.R, G = p.G, S = p.S;
    const int psA = (2 * R + p.coutp) * 16, psZ = G * 16;
    float* BA = lds;
    float* Z = BA + NT * psA;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kl = lane >> 4, j = lane & 15;
    const long long N = p.N;
    const auto ident = [](int k) { return k; };
    long long b;
    int p0;
    tile_of_block(p, TN, b, p0);

    const float* hb = p.hin + b * R * N;
    stage_rows(BA, psA, 0, R, NT, hb, R, N, p0, p.dil, tid);
    stage_rows(BA, psA, R, R, NT, hb, R, N, p0, 0, tid);
    stage_rows(BA, psA, 2 * R, p.coutp, NT, p.cfeat + b * p.cout * N, p.cout, N, p0, 0, tid);
    __syncthreads();

    for (int t = wave; t < G / 16; t += WAVES) {
        f32x4 acc[2][NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            acc[0][nt] = acc[1][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        const f32x4 bf = bias_tile(p.b1, t, lane);
        const f32x4 bg = bias_tile(p.b1 + G, t, lane);
        const float4* base = p.w1 + ((long long)t * 2) * p.K1q * 64;
        const float4* const A[2] = {base, base + (long long)p.K1q * 64};
        gemm<2, NT>(A, p.K1q, BA, psA, ident, lane, acc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (SAVE) {
                    const float tv = tanh_e(acc[0][nt][r] + bf[r]), sv = sigmoid_e(acc[1][nt][r] + bg[r]);
                    const int g = t * 16 + 4 * kl + r;
                    const long long pos = p0 + nt * 16 + j;
                    Z[nt * psZ + g * 16 + j] = tv * sv;
                    if (pos < N) {
                        p.ts[(b * 2 * G + g) * N + pos] = tv;
                        p.ts[(b * 2 * G + G + g) * N + pos] = sv;
                    }
                } else {
                    Z[nt * psZ + (t * 16 + 4 * kl + r) * 16 + j] = tanh_e(acc[0][nt][r] + bf[r]) * sigmoid_e(acc[1][nt][r] + bg[r]);
                }
            }
    }
    __syncthreads();

    const int rt = p.last ? 0 : R / 16;  // the last block's residual output is never read
    for (int u = wave; u < rt + S / 16; u += WAVES) {
        f32x4 acc[1][NT];
        if (u < rt) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[0][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const f32x4 bias = bias_tile(p.b_res, u, lane);
            const float4* const A[1] = {p.w2 + (long long)u * p.Gq * 64};
            gemm<1, NT>(A, p.Gq, Z, psZ, ident, lane, acc);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = u * 16 + 4 * kl + r;
                    const long long pos = p0 + nt * 16 + j;
                    const float h = BA[nt * psA + (R + row) * 16 + j];
                    if (pos < N) p.hout[(b * R + row) * N + pos] = (h + (acc[0][nt][r] + bias[r])) * 0.70710678118654752f;
                }
        } else {
            const int t = u - rt;
            float* sk = p.skip + (b * S + t * 16 + 4 * kl) * N + p0 + j;  // + r * N + nt * 16
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[0][nt][r] = (!p.first && p0 + nt * 16 + j < N) ? sk[r * N + nt * 16] : 0.0f;
            const float4* const A[1] = {p.w2 + (long long)(R / 16 + t) * p.Gq * 64};
            gemm<1, NT>(A, p.Gq, Z, psZ, ident, lane, acc);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (p0 + nt * 16 + j < N) sk[r * N + nt * 16] = acc[0][nt][r];
        }
    }
}

// ReLU, 1x1 S->S, ReLU, 1x1 S->2 (wavenet.py:50-56).  LDS: Z [TN/16][S][16] relu(skip + b_skip), O [TN/16][S][16].
// SAVE: O also goes to p.osave.
template <int TN, bool SAVE = false>
__global__ __launch_bounds__(THREADS) void k_wnf_final(const ForwardParams p) {
    constexpr int NT = TN / 16;
    extern __shared__ float lds[];
    const int S = p.S, psS = S * 16;
    float* Z = lds;
    float* O = Z + NT * psS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kl = lane >> 4, j = lane & 15;
    const long long N = p.N;
    const auto ident = [](int k) { return k; };
    long long b;
    int p0;
    tile_of_block(p, TN, b, p0);
    for (int l = tid; l < NT * psS; l += THREADS) {
        const int nt = l / psS, row = (l - nt * psS) >> 4;
        const long long pos = (long long)p0 + nt * 16 + (l & 15);
        Z[l] = pos < N ? fmaxf(p.skip[(b * S + row) * N + pos] + p.b_skip[row], 0.0f) : 0.0f;
    }
    __syncthreads();
    for (int t = wave; t < S / 16; t += WAVES) {
        f32x4 acc[1][NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[0][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 bias = bias_tile(p.b_f1, t, lane);
        const float4* const A[1] = {p.w_f1 + (long long)t * p.Sq * 64};
        gemm<1, NT>(A, p.Sq, Z, psS, ident, lane, acc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float o = fmaxf(acc[0][nt][r] + bias[r], 0.0f);
                O[nt * psS + (t * 16 + 4 * kl + r) * 16 + j] = o;
                if constexpr (SAVE) {
                    const long long pos = p0 + nt * 16 + j;
                    if (pos < N) p.osave[(b * S + t * 16 + 4 * kl + r) * N + pos] = o;
                }
            }
    }
    __syncthreads();
    for (int nt = wave; nt < NT; nt += WAVES) {  // rows 0 and 1 (mean, log_std) of N tile nt land in lanes 0..15
        f32x4 acc[1][1];
        acc[0][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float4* const A[1] = {p.w_f2};
        gemm<1, 1>(A, p.Sq, O + nt * psS, 0, ident, lane, acc);
        const long long pos = (long long)p0 + nt * 16 + lane;
        if (lane < 16 && pos < N) {
            p.stats[(b * N + pos) * 2] = acc[0][0][0] + p.b_f2[0];
            p.stats[(b * N + pos) * 2 + 1] = acc[0][0][1] + p.b_f2[1];
        }
    }
}

}  // namespace fpc_wn

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
