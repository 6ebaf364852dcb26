// wavenet_decode.h -- k_wn_decode: the sample loop of the Gaussian WaveNet vocoder (src/models/wavenet.py:137-193,
// src/models/modules.py:36-86) as one persistent workgroup per tile of NU utterances (gfx950).
//
// Work split.  A workgroup of 16 wavefronts owns NU (16 or 32) utterances and walks all samples alone: no exchange between
// workgroups, no spinning, no residency assumption.  Per sample every layer is two dense products on
// v_mfma_f32_16x16x4_f32, output channels on M, utterances on N:
//   GEMM1  [2G x (2R + cout)] . [(2R + cout) x NU]   K = [h(p - dil) | h(p) | c(p)]: both taps and the conditioning in one K
//   GEMM2  [(R + S) x G] . [G x NU]                  rows [0,R) the residual, [R,R+S) the skip convolution
// A wavefront owns whole 16-row M tiles (tile t, t + 16, ...).  In GEMM1 it carries the filter tile and the gate tile of the same
// 16 channels side by side, so that one B fragment feeds both and z = tanh(f) * sigmoid(g) is formed in the accumulator
// registers; with NU = 32 the two N tiles share every A fragment.
//
// Weights are prepacked at create time in the per-lane order of the MFMA A operand, four k-steps to a 16-byte word:
//   word[(tile * KQ + q) * 64 + lane].comp[i] = A[tile * 16 + lane % 16][q * 16 + i * 4 + lane / 16]
// so a wavefront streams a tile as consecutive 1 KiB rows (global_load_dwordx4), the next word in flight while the four
// MFMAs of the current one issue; sixteen wavefronts keep sixteen such streams going.  Nothing on chip holds the weights
// (21 MB at the configured shape): they come from L2 / the memory-side cache every sample.
//
// LDS map (floats; a "panel" is [rows][16], one per N tile, so that the B-operand read of a k-step -- rows 4k..4k+3, 16
// columns -- is 64 consecutive floats: conflict-free):
//   BA  [NT][rowsA][16]  rows [0,R) h(p - dil), [R,2R) h(p), [2R,2R+coutp) c(p); the last stage reuses rows [0,S)
//   Z   [NT][rowsZ][16]  z of the layer; relu(skip) in the last stage
//   XH  [NT][inp*32][16] the last 32 inputs of each input channel, a ring indexed by position & 31
//   LP  [NT][16][16]     the 16 LPC taps of the current frame, per utterance
// Registers: the skip accumulator never leaves the MFMA accumulators of the wavefront that owns its tile (two tiles per
// wavefront at most: S <= 512); x(i-1) and pred(i) of an utterance live in the lane that samples it.
// The dilation queues are rings in the workspace, per layer `dil` columns of [R][NU]; a step touches one column per layer:
// the slot read as h(p - dil) is then overwritten with h(p).
//
// Accumulation order over K is fixed (k ascending from zero, the bias last) and columns never mix, so an utterance's output depends
// neither on B nor on its column nor on NU.
//
// Noise.  eps comes from the caller's buffer, or from Philox4x32-10 with key = the utterance's 64-bit seed and counter
// (i, 0, 0, 0): with (c0, c1) the first two output words,
//   u1 = ((c0 >> 9) + 0.5) * 2^-23,  u2 = (c1 >> 8) * 2^-24,  eps = sqrt(-2 ln u1) * cos(2 pi u2)      (Box-Muller)
// ln is fpc_logf, sqrt the IEEE one, cos the device library's cospif(2 u2).
#pragma once
#include "fpc_common.h"

// Packed fp32 code generation (v_pk_mul_f32, v_pk_fma_f32) is off for every function of this header, as the Makefile has it
// for bitstream.hip; the region closes at the end of the file.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace fpc_wn {

constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int FRONT = 32;           // taps of the front convolution (wavenet.py:36)
constexpr int MAX_SKIP_TILES = 2;   // per wavefront: S <= 512

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DecodeParams {
    int B, N, T;                      // utterances, samples (160 T), frames
    int R, G, S, cout, coutp, inp, layers;
    int K0q, K1q, Gq, Sq;             // 16-wide K groups of the front layer, GEMM1, GEMM2, the last stage
    int rowsA, rowsZ;                 // panel heights
    const float4* w_front;            // [R/16][K0q][64]
    const float* b_front;             // [R]
    const float4* w1;                 // [layers][G/16][2][K1q][64]   filter tile, gate tile
    const float* b1;                  // [layers][2][G]               conv bias + conditioning bias
    const float4* w2;                 // [layers][(R+S)/16][Gq][64]
    const float* b_res;               // [layers][R]
    const float* b_skip;              // [S] summed over the layers
    const float4* w_f1;               // [S/16][Sq][64]
    const float* b_f1;                // [S]
    const float4* w_f2;               // [1][Sq][64] rows 0,1 = mean, log_std; the other 14 rows zero
    float b_f2[2];
    const int* dil;                   // [layers]
    const long long* ring_off;        // [layers] first column of the layer's ring
    float* ring;                      // [tiles][sum dil][R][NU]
    long long ring_cols;              // sum dil
    const float* cfeat;               // [tiles][N][cout][NU], columns past B zero (k_wn_upsample)
    const float* lpc;                 // [B][T][16]
    const unsigned long long* seeds;  // [B]
    const float* noise;               // [B][N] or null
    const float* xin;                 // [B][N]: teacher-forced, else null
    float* out;                       // [B][N]     (free run)
    float* xout;                      // [B][N] or null: x itself (free run)
    float* stats;                     // [B][N][2]  (teacher-forced)
};

__device__ __forceinline__ void philox2(unsigned long long seed, uint32_t t, uint32_t& o0, uint32_t& o1) {
    uint32_t c0 = t, c1 = 0u, c2 = 0u, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = fpc_mulhi32(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = fpc_mulhi32(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0;
        c1 = l1;
        c2 = n2;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o0 = c0;
    o1 = c1;
}

__device__ __forceinline__ float gaussian(unsigned long long seed, uint32_t i) {
    uint32_t c0, c1;
    philox2(seed, i, c0, c1);
    const float u1 = ((float)(c0 >> 9) + 0.5f) * 1.1920928955078125e-07f;  // 2^-23
    const float u2 = (float)(c1 >> 8) * 5.9604644775390625e-08f;           // 2^-24
    return sqrtf(-2.0f * fpc_logf(u1)) * cospif(2.0f * u2);
}

// tanh and the logistic for a check against float64 (tests/test_gpu_wavenet.py): relative error below 1.5e-7 everywhere,
// where the rational fpc_tanhf is 3e-7 absolute.  Below 0.625 the odd polynomial of Cephes' tanhf (small outputs keep their
// relative accuracy: the upsampler scales them down further); above, exp(-2|x|) with an IEEE quotient.
__device__ __forceinline__ float tanh_e(float x) {
    const float a = fabsf(x);
    if (a < 0.625f) {
        const float z = x * x;
        float p = fmaf(-5.70498872745e-3f, z, 2.06390887954e-2f);
        p = fmaf(p, z, -5.37397155531e-2f);
        p = fmaf(p, z, 1.33314422036e-1f);
        p = fmaf(p, z, -3.33332819422e-1f);
        return fmaf(x * z, p, x);
    }
    const float e = fpc_expf(-2.0f * a);
    return copysignf((1.0f - e) / (1.0f + e), x);
}
__device__ __forceinline__ float sigmoid_e(float x) { return 1.0f / (1.0f + fpc_expf(-x)); }

// one tap of the prediction's sum (utils.py:91-114): s = 0, then k ascending over the 16 taps, pred = -s.  The sample loop and
// k_wnf_inputs (wavenet_forward.h) both compile this expression.  (The whole loop in a shared function changed the register
// allocation of k_wn_decode<32>; the tap alone leaves both instances' code as it was.)
__device__ __forceinline__ float lpc_tap(float s, float a, float x) { return s + a * x; }

// acc[a][nt] += A_a[16 x 16 KQ] . B[16 KQ x 16 nt..]: NA weight tiles against the same B fragments.  `row` maps a K index to
// its panel row.
template <int NA, int NT, class RowFn>
__device__ __forceinline__ void gemm(const float4* const (&A)[NA], int KQ, const float* Bp, int pstride, RowFn row, int lane,
                                     f32x4 (&acc)[NA][NT]) {
    const int kl = lane >> 4, j = lane & 15;
    float4 cur[NA], nxt[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) cur[a] = A[a][lane];
    for (int q = 0; q < KQ; ++q) {
        const int qn = q + 1 < KQ ? q + 1 : q;
#pragma unroll
        for (int a = 0; a < NA; ++a) nxt[a] = A[a][qn * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = row(q * 16 + i * 4 + kl) * 16 + j;
            float b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = Bp[nt * pstride + r];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const float av = i == 0 ? cur[a].x : i == 1 ? cur[a].y : i == 2 ? cur[a].z : cur[a].w;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[a][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[nt], acc[a][nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) cur[a] = nxt[a];
    }
}

// the bias of an accumulator tile, added after the sum as torch's convolutions do (where a bias dominates the sum, adding
// it first would round every partial sum at the bias's magnitude): element r of a lane is row 4 (lane / 16) + r of the tile
__device__ __forceinline__ f32x4 bias_tile(const float* b, int tile, int lane) {
    const float* s = b + tile * 16 + 4 * (lane >> 4);
    f32x4 v = {s[0], s[1], s[2], s[3]};
    return v;
}

template <int NU>
__global__ __launch_bounds__(THREADS) void k_wn_decode(const DecodeParams p) {
    constexpr int NT = NU / 16;
    extern __shared__ float lds[];
    const int psA = p.rowsA * 16, psZ = p.rowsZ * 16, psX = p.inp * FRONT * 16;
    float* BA = lds;
    float* Z = BA + NT * psA;
    float* XH = Z + NT * psZ;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kl = lane >> 4, j = lane & 15;
    const int R = p.R, G = p.G, S = p.S;
    const long long N = p.N;
    const auto ident = [](int k) { return k; };

    float* LP = XH + NT * psX;
    for (int e = tid; e < NT * (psA + psZ + psX + 256); e += THREADS) lds[e] = 0.0f;

    // the lane that samples an utterance: lanes 0..15 of wavefront nt hold the columns of N tile nt after the last product
    const bool sampler = wave < NT && lane < 16;
    const int col = wave * 16 + lane;
    const long long ub = (long long)blockIdx.x * NU + col;
    const bool live = sampler && ub < p.B;
    float xprev = 0.0f, pred = 0.0f;
    const unsigned long long seed = (live && p.seeds) ? p.seeds[ub] : 0ull;
    float* xh_col = XH + (sampler ? wave * psX + lane : 0);  // + (channel * 32 + slot) * 16
    float* lp_col = LP + (sampler ? wave * 256 + lane : 0);  // + tap * 16

    f32x4 skip[MAX_SKIP_TILES][1][NT];
    float* ring_tile = p.ring + (long long)blockIdx.x * p.ring_cols * R * NU;
    __syncthreads();

    for (int i = 0; i < p.N; ++i) {
        // ---- 0: prediction of sample i from the utterance's own history (utils.py:91-114), conditioning column ----
        if (sampler) {
            if (live && i % 160 == 0) {
                const float* a = p.lpc + (ub * p.T + i / 160) * 16;
#pragma unroll
                for (int k = 0; k < 16; ++k) lp_col[k * 16] = a[k];
            }
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s = lpc_tap(s, lp_col[k * 16], xh_col[((i - k) & 31) * 16]);  // x(i-1-k) sits at position i-k
            pred = -s;
            if (p.inp == 3) xh_col[(2 * FRONT + (i & 31)) * 16] = pred;
        }
        {  // the step's cout x NU conditioning values are one contiguous block
            const float* cf = p.cfeat + ((long long)blockIdx.x * N + i) * p.cout * NU;
            for (int e = tid; e < p.cout * NU; e += THREADS) {
                const int ch = e / NU, c = e % NU;
                BA[(c >> 4) * psA + (2 * R + ch) * 16 + (c & 15)] = cf[e];
            }
        }
        __syncthreads();

        // ---- 1: front convolution over the last 32 inputs + ReLU (wavenet.py:37-40) -> h(p) ----
        for (int t = wave; t < R / 16; t += WAVES) {
            f32x4 acc[1][NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[0][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const f32x4 bias = bias_tile(p.b_front, t, lane);
            const float4* const A[1] = {p.w_front + (long long)t * p.K0q * 64};
            // tap k of channel c multiplies the input at position i - 31 + k, ring slot (i + 1 + k) & 31
            gemm<1, NT>(A, p.K0q, XH, psX, [i](int k) { return (k & ~31) | ((i + 1 + k) & 31); }, lane, acc);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    BA[nt * psA + (R + t * 16 + 4 * kl + r) * 16 + j] = fmaxf(acc[0][nt][r] + bias[r], 0.0f);
        }
#pragma unroll
        for (int ti = 0; ti < MAX_SKIP_TILES; ++ti)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) skip[ti][0][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        __syncthreads();

        // ---- 2: the residual blocks (modules.py:62-77) ----
        for (int n = 0; n < p.layers; ++n) {
            {  // queue: the slot holds h(p - dil); it gets h(p)
                const int d = p.dil[n];
                float* slot = ring_tile + (p.ring_off[n] + (i & (d - 1))) * R * NU;
                for (int e = tid; e < R * NU; e += THREADS) {
                    const int r = e / NU, c = e % NU;
                    const int at = (c >> 4) * psA + r * 16 + (c & 15);
                    const float old = slot[e];
                    slot[e] = BA[at + R * 16];
                    BA[at] = old;
                }
            }
            __syncthreads();
            for (int t = wave; t < G / 16; t += WAVES) {
                f32x4 acc[2][NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc[0][nt] = acc[1][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
                const f32x4 bf = bias_tile(p.b1 + (long long)n * 2 * G, t, lane);
                const f32x4 bg = bias_tile(p.b1 + (long long)n * 2 * G + G, t, lane);
                const float4* base = p.w1 + (((long long)n * (G / 16) + t) * 2) * p.K1q * 64;
                const float4* const A[2] = {base, base + (long long)p.K1q * 64};
                gemm<2, NT>(A, p.K1q, BA, psA, ident, lane, acc);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        Z[nt * psZ + (t * 16 + 4 * kl + r) * 16 + j] = tanh_e(acc[0][nt][r] + bf[r]) * sigmoid_e(acc[1][nt][r] + bg[r]);
            }
            __syncthreads();
            const float4* w2n = p.w2 + (long long)n * ((R + S) / 16) * p.Gq * 64;
            if (n + 1 < p.layers)  // the last block's residual output is never read
                for (int t = wave; t < R / 16; t += WAVES) {
                    f32x4 acc[1][NT];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[0][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    const f32x4 bias = bias_tile(p.b_res + (long long)n * R, t, lane);
                    const float4* const A[1] = {w2n + (long long)t * p.Gq * 64};
                    gemm<1, NT>(A, p.Gq, Z, psZ, ident, lane, acc);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float* h = BA + nt * psA + (R + t * 16 + 4 * kl + r) * 16 + j;
                            *h = (*h + (acc[0][nt][r] + bias[r])) * 0.70710678118654752f;
                        }
                }
#pragma unroll
            for (int ti = 0; ti < MAX_SKIP_TILES; ++ti) {
                const int t = wave + ti * WAVES;
                if (t < S / 16) {
                    const float4* const A[1] = {w2n + (long long)(R / 16 + t) * p.Gq * 64};
                    gemm<1, NT>(A, p.Gq, Z, psZ, ident, lane, skip[ti]);
                }
            }
            __syncthreads();
        }

        // ---- 3: ReLU, 1x1 S->S, ReLU, 1x1 S->2 (wavenet.py:50-56) ----
#pragma unroll
        for (int ti = 0; ti < MAX_SKIP_TILES; ++ti) {
            const int t = wave + ti * WAVES;
            if (t < S / 16) {
                const f32x4 bias = bias_tile(p.b_skip, t, lane);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        Z[nt * psZ + (t * 16 + 4 * kl + r) * 16 + j] = fmaxf(skip[ti][0][nt][r] + bias[r], 0.0f);
            }
        }
        __syncthreads();
        for (int t = wave; t < S / 16; t += WAVES) {
            f32x4 acc[1][NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[0][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const f32x4 bias = bias_tile(p.b_f1, t, lane);
            const float4* const A[1] = {p.w_f1 + (long long)t * p.Sq * 64};
            gemm<1, NT>(A, p.Sq, Z, psZ, ident, lane, acc);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) BA[nt * psA + (t * 16 + 4 * kl + r) * 16 + j] = fmaxf(acc[0][nt][r] + bias[r], 0.0f);
        }
        __syncthreads();
        if (wave < NT) {  // wavefront nt: the two output rows of N tile nt; rows 0 and 1 land in lanes 0..15
            f32x4 acc[1][1];
            acc[0][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const float4* const A[1] = {p.w_f2};
            gemm<1, 1>(A, p.Sq, BA + wave * psA, 0, ident, lane, acc);
            if (sampler) {
                const float mean = acc[0][0][0] + p.b_f2[0], ls = acc[0][0][1] + p.b_f2[1];
                float x = 0.0f, exc = 0.0f;
                if (live) {
                    if (p.xin) {
                        p.stats[(ub * N + i) * 2] = mean;
                        p.stats[(ub * N + i) * 2 + 1] = ls;
                        x = p.xin[ub * N + i];
                        exc = x - pred;
                    } else {
                        const float eps = p.noise ? p.noise[ub * N + i] : gaussian(seed, (uint32_t)i);
                        exc = mean + fpc_expf(ls) * eps;  // utils.py:33-43
                        x = exc + pred;                   // wavenet.py:183
                        p.out[ub * N + i] = 0.85f * xprev + x;  // wavenet.py:188, as written
                        if (p.xout) p.xout[ub * N + i] = x;
                    }
                }
                xprev = x;
                xh_col[((i + 1) & 31) * 16] = x;  // the net sees x(i) at position i + 1
                if (p.inp == 3) xh_col[(FRONT + ((i + 1) & 31)) * 16] = exc;
            }
        }
        __syncthreads();
    }
}

// the dilation queues start as zeros: each layer zero-pads its own input (modules.py:17, 22)
__global__ __launch_bounds__(256) void k_wn_clear(float4* p, long long n4) {
    const float4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long long)gridDim.x * 256) p[e] = z;
}

}  // namespace fpc_wn

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
