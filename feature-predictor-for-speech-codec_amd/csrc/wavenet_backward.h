// wavenet_backward.h -- k_wnb_*: the Gaussian loss (src/loss.py:6-21 as src/train.py:139 calls it) and the backward pass of the
// teacher-forced WaveNet (wavenet.py:50-56, modules.py:62-77) over all positions at once (gfx950).
//
// The forward runs first as the SAVE instances of k_wnf_layer / k_wnf_final (wavenet_forward.h).  Stored per layer: the layer's
// input h [B][R][N] (one buffer per layer instead of the ping-pong pair) and t = tanh(a_f), s = sigmoid(a_g) [B][2G][N]; once:
// the skip sum, the last stage's hidden output o and the stats.  z = t s is formed again where it is read, relu(skip + b_skip)
// likewise: neither is stored.
//
//   k_wnb_loss      nll and its sum, fixed order in float64; dstats [B][2][N] (planar: the two rows are an A operand later)
//   k_wnb_final     dstats -> do1 = (W_f2^T dstats)[o > 0] -> dskip = (W_f1^T do1)[skip + b_skip > 0]
//   k_wnb_layer     one residual block, walked from the last to the first (one launch per block)
//   k_wnb_front     dpre0 = dh0 [h0 > 0]
//   k_wnb_wgrad     every weight gradient: positions on the K side of the MFMA; k_wnb_reduce adds its segments
//
// k_wnb_layer: time on the N side of v_mfma_f32_16x16x4_f32, a workgroup of 16 wavefronts owns one utterance x TN positions
// as in the forward, the weights are the transposed tiles packed at create (w2t, w1t) and run through the forward's `gemm`.
// LDS (floats, panels [rows][16] per N tile):
//   D   [TN/16][R + S][16]   rows [0,R) sqrt(1/2) dh'(p), [R,R+S) dskip(p)
//   DA  [TN/16][2G][16]      rows [0,G) da_f, [G,2G) da_g
// (R + S + 2G) TN floats: 96 KiB at TN = 32, 48 KiB at TN = 16 for R/G/S 128/256/128.
//   stage   dh'(p) = DH(p) + E0(p + d_next) of the block after this one (zero for the last block, zero where p + d_next >= N);
//           the scaled panel rows also go to `dhp`, the left operand of the res_conv weight gradient
//   GEMM1   dz tile [16 x TN] = W2^T [G x (R+S)] . D; a wavefront owns 16 gate channels and forms da_f = dz s (1 - t^2),
//           da_g = dz t s (1 - s) in its accumulators -> DA and `da` [B][2G][N] (left operand of the W1 weight gradient)
//   GEMM2   [(2R + coutp) x 2G] . DA: rows [0,R) -> E0 (unshifted), rows [R,2R) + sqrt(1/2) dh' -> DH, rows [2R,..) take the
//           running dc from the cfeat gradient as the MFMA's C operand and store it back
// The shifted tap crosses time tiles through the launch boundary only, as h(p - dil) does in the forward.
//
// k_wnb_wgrad: dW[M x K] = sum over (b, p) of A[m][b,p] Bop[k][b,p].  One wavefront per workgroup owns a 64 x 64 block of dW
// (4 x 4 MFMA tiles: a loaded 16-byte word feeds four MFMAs, 0.5 loads per MFMA) over one segment of the positions; both
// operands are read row-major with p contiguous, a lane's word is four k-steps.  Operand rows are described by up to three
// row groups (WgRows): a plain buffer read at p - shift (h(p - d), h(p), cfeat; the front convolution's Toeplitz read is a
// plain row with a shift per row), t s formed on load, or relu(skip + b_skip).  Partial sums go to the workspace and
// k_wnb_reduce adds the segments in ascending order, in float64, and writes PyTorch's layouts: no float atomics, same bits
// every run.  The bias sums are the row sums of A: k_wnb_rowsum, one workgroup per row, float64, a fixed tree.  (Measured: as
// four more MFMAs against a B operand of ones in the wavefronts of K block 0 the sum of 160 same-signed terms missed the
// test's bound by 3 ulp; a float32 chain over the positions cannot do better.)
#pragma once
#include "wavenet_forward.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace fpc_wn {

constexpr float SQRT_HALF = 0.70710678118654752f;

struct BackwardParams {
    int B, N, tiles;
    int R, G, S, cout, coutp;
    int K2q, K1q, Sq;                 // 16-wide K groups: (R+S)/16 of GEMM1, 2G/16 of GEMM2, S/16 of the last stage
    int n_valid;
    double inv_m;                     // 1 / (B n_valid)
    const float* stats;               // [B][N][2]
    const float* target;              // [B][N]
    float* dstats;                    // [B][2][N]
    double* lossb;                    // [B]
    float* loss;                      // [1]
    const float* f2;                  // [2][S] final2_w, plain
    const float4* w_f1t;              // [S/16][Sq][64]
    const float* osave;               // [B][S][N]
    const float* skip;                // [B][S][N]
    const float* b_skip;              // [S]
    float* do1;                       // [B][S][N]
    float* dskip;                     // [B][S][N]
    const float4* w2t;                // [G/16][K2q][64] of THIS layer
    const float4* w1t;                // [(2R+coutp)/16][K1q][64]
    const float* ts;                  // [B][2G][N] of this layer
    const float* dh_in;               // [B][R][N] DH of the block after this one
    const float* e0_in;               // [B][R][N] E0 of the block after this one
    int dil_next, last, first;        // last block: dh' = 0; first launch: dc starts at zero
    float* dhp;                       // [B][R][N] sqrt(1/2) dh'
    float* da;                        // [B][2G][N]
    float* dh_out;                    // [B][R][N]
    float* e0_out;                    // [B][R][N]
    float* dc;                        // [B][cout][N]
    const float* h0;                  // [B][R][N] (k_wnb_front)
    float* dpre0;                     // [B][R][N]
};

// One workgroup per utterance.  nll in float64 from the float32 stats; threads stride over the positions, then a fixed tree.
__global__ __launch_bounds__(256) void k_wnb_loss(const BackwardParams p) {
    __shared__ double red[256];
    const long long b = blockIdx.x, N = p.N;
    double acc = 0.0;
    for (int i = threadIdx.x; i < p.N; i += 256) {
        float dm = 0.0f, dl = 0.0f;
        if (i < p.n_valid) {
            const float mean = p.stats[(b * N + i) * 2], raw = p.stats[(b * N + i) * 2 + 1];
            const double ls = raw > -9.0f ? (double)raw : -9.0, e = (double)p.target[b * N + i] - (double)mean;
            const double w = exp(-2.0 * ls), q = e * e * w;
            acc += 0.5 * (1.8378770664093454836 + 2.0 * ls + q);
            dm = (float)(-e * w * p.inv_m);
            dl = raw > -9.0f ? (float)((1.0 - q) * p.inv_m) : 0.0f;
        }
        p.dstats[(b * 2) * N + i] = dm;
        p.dstats[(b * 2 + 1) * N + i] = dl;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.lossb[b] = red[0];
}

// the utterances in sequence
__global__ void k_wnb_loss_sum(const BackwardParams p) {
    double a = 0.0;
    for (int b = 0; b < p.B; ++b) a += p.lossb[b];
    *p.loss = (float)(a * p.inv_m);
}

// LDS: P [TN/16][S][16] do1.  The S -> 2 product has K = 2: plain FMAs.
template <int TN>
__global__ __launch_bounds__(THREADS) void k_wnb_final(const BackwardParams p) {
    constexpr int NT = TN / 16;
    extern __shared__ float lds[];
    const int S = p.S, psS = S * 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kl = lane >> 4, j = lane & 15;
    const long long N = p.N, b = blockIdx.x / p.tiles;
    const int p0 = (int)(blockIdx.x % p.tiles) * TN;
    const auto ident = [](int k) { return k; };
    for (int l = tid; l < NT * psS; l += THREADS) {
        const int nt = l / psS, row = (l - nt * psS) >> 4;
        const long long pos = (long long)p0 + nt * 16 + (l & 15);
        float v = 0.0f;
        if (pos < N) {
            const float d = p.f2[row] * p.dstats[(b * 2) * N + pos] + p.f2[S + row] * p.dstats[(b * 2 + 1) * N + pos];
            v = p.osave[(b * S + row) * N + pos] > 0.0f ? d : 0.0f;
            p.do1[(b * S + row) * N + pos] = v;
        }
        lds[l] = v;
    }
    __syncthreads();
    for (int t = wave; t < S / 16; t += WAVES) {
        f32x4 acc[1][NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[0][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float4* const A[1] = {p.w_f1t + (long long)t * p.Sq * 64};
        gemm<1, NT>(A, p.Sq, lds, psS, ident, lane, acc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = t * 16 + 4 * kl + r;
                const long long pos = p0 + nt * 16 + j;
                if (pos < N) {
                    const long long at = (b * S + row) * N + pos;
                    p.dskip[at] = p.skip[at] + p.b_skip[row] > 0.0f ? acc[0][nt][r] : 0.0f;
                }
            }
    }
}

template <int TN>
__global__ __launch_bounds__(THREADS) void k_wnb_layer(const BackwardParams p) {
    constexpr int NT = TN / 16;
    extern __shared__ float lds[];
    const int R = p.R, G = p.G, S = p.S;
    const int psD = (R + S) * 16, psA = 2 * G * 16;
    float* D = lds;
    float* DA = D + NT * psD;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kl = lane >> 4, j = lane & 15;
    const long long N = p.N, b = blockIdx.x / p.tiles;
    const int p0 = (int)(blockIdx.x % p.tiles) * TN;
    const auto ident = [](int k) { return k; };

    for (int l = tid; l < NT * R * 16; l += THREADS) {
        const int nt = l / (R * 16), rem = l - nt * R * 16, row = rem >> 4;
        const long long pos = (long long)p0 + nt * 16 + (rem & 15);
        float v = 0.0f;
        if (pos < N) {
            if (!p.last) {
                const long long at = (b * R + row) * N + pos;
                v = p.dh_in[at];
                if (pos + p.dil_next < N) v += p.e0_in[at + p.dil_next];
                v *= SQRT_HALF;
            }
            p.dhp[(b * R + row) * N + pos] = v;
        }
        D[nt * psD + rem] = v;
    }
    stage_rows(D, psD, R, S, NT, p.dskip + b * S * N, S, N, p0, 0, tid);
    __syncthreads();

    for (int t = wave; t < G / 16; t += WAVES) {
        f32x4 acc[1][NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[0][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float4* const A[1] = {p.w2t + (long long)t * p.K2q * 64};
        gemm<1, NT>(A, p.K2q, D, psD, ident, lane, acc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int g = t * 16 + 4 * kl + r;
                const long long pos = p0 + nt * 16 + j;
                float df = 0.0f, dg = 0.0f;
                if (pos < N) {
                    const long long at = (b * 2 * G + g) * N + pos;
                    const float tv = p.ts[at], sv = p.ts[at + G * N], dz = acc[0][nt][r];
                    df = dz * sv * (1.0f - tv * tv);
                    dg = dz * tv * sv * (1.0f - sv);
                    p.da[at] = df;
                    p.da[at + G * N] = dg;
                }
                DA[nt * psA + g * 16 + j] = df;
                DA[nt * psA + (G + g) * 16 + j] = dg;
            }
    }
    __syncthreads();

    const int rt = R / 16;
    for (int u = wave; u < 2 * rt + p.coutp / 16; u += WAVES) {
        f32x4 acc[1][NT];
        const int c0 = (u - 2 * rt) * 16 + 4 * kl;  // conditioning row of element r = 0
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long pos = p0 + nt * 16 + j;
                const bool take = u >= 2 * rt && !p.first && c0 + r < p.cout && pos < N;
                acc[0][nt][r] = take ? p.dc[(b * p.cout + c0 + r) * N + pos] : 0.0f;
            }
        const float4* const A[1] = {p.w1t + (long long)u * p.K1q * 64};
        gemm<1, NT>(A, p.K1q, DA, psA, ident, lane, acc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long pos = p0 + nt * 16 + j;
                if (pos >= N) continue;
                if (u < rt) {
                    p.e0_out[(b * R + u * 16 + 4 * kl + r) * N + pos] = acc[0][nt][r];
                } else if (u < 2 * rt) {
                    const int row = (u - rt) * 16 + 4 * kl + r;
                    p.dh_out[(b * R + row) * N + pos] = acc[0][nt][r] + D[nt * psD + row * 16 + j];
                } else if (c0 + r < p.cout) {
                    p.dc[(b * p.cout + c0 + r) * N + pos] = acc[0][nt][r];
                }
            }
    }
}

// dpre0 = (DH(p) + E0(p + d_0)) [h0 > 0] of the first block's outputs
__global__ __launch_bounds__(256) void k_wnb_front(const BackwardParams p) {
    const long long N = p.N, total = (long long)p.B * p.R * N;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long pos = idx % N;
        float v = p.dh_in[idx];
        if (pos + p.dil_next < N) v += p.e0_in[idx + p.dil_next];
        p.dpre0[idx] = p.h0[idx] > 0.0f ? v : 0.0f;
    }
}

// ---- weight gradients ----

enum { WG_PLAIN = 0, WG_PRODUCT = 1, WG_RELU_BIAS = 2 };

// `rows` operand rows (a multiple of 16) from one source: row r < valid reads src[b * bstride + (r / div) * N + p - shift],
// shift = shift0 + shift_step * (r % div); rows >= valid, and positions before the utterance, are zero.  div = 32 with
// shift_step = -1 is the front convolution's Toeplitz read (row = channel * 32 + tap), div = 1 a plain row.
struct WgRows {
    const float* src;
    long long bstride;
    int rows, valid, shift0, shift_step, div, mode;
    long long aux_off;   // WG_PRODUCT: the second factor's offset from the first
    const float* bias;   // WG_RELU_BIAS: [valid]
};
struct WgSide {
    WgRows g[3];
    int total;  // rows of the operand, a multiple of 16
};
struct WgradParams {
    WgSide a, bop;
    int N, chunks, cps;      // 16-position chunks in all (B N / 16) and per segment
    int mblocks, kblocks;    // 64-row blocks of dW
    float* part;             // [segs][mblocks 64][kblocks 64]
};

struct WgLane {        // one operand row as the lane reading it sees it
    const float* ptr;  // the row at position 0 of utterance 0; null: a zero row
    long long bstride, aux_off;
    int shift, mode;
    float bias;
};

__device__ __forceinline__ WgLane wg_resolve(const WgSide& s, int row, long long N) {
    int base = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const WgRows& g = s.g[i];
        const int r = row - base;
        if (r >= 0 && r < g.rows) {
            if (r >= g.valid) break;
            return WgLane{g.src + (long long)(r / g.div) * N, g.bstride, g.aux_off, g.shift0 + g.shift_step * (r % g.div), g.mode,
                          g.mode == WG_RELU_BIAS ? g.bias[r] : 0.0f};
        }
        base += g.rows;
    }
    return WgLane{nullptr, 0, 0, 0, WG_PLAIN, 0.0f};
}

// the row's values at positions p .. p + 3 of utterance b (p a multiple of 4, p + 3 < N since N is a multiple of 16)
__device__ __forceinline__ f32x4 wg_fetch(const WgLane& t, long long b, int p) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t.ptr == nullptr) return v;
    const float* s = t.ptr + b * t.bstride;
    const int q = p - t.shift;
    if ((t.shift & 3) == 0) {
        if (q < 0) return v;
        const float4 w = *reinterpret_cast<const float4*>(s + q);
        v = f32x4{w.x, w.y, w.z, w.w};
        if (t.mode == WG_PRODUCT) {
            const float4 u = *reinterpret_cast<const float4*>(s + t.aux_off + q);
            v = f32x4{w.x * u.x, w.y * u.y, w.z * u.z, w.w * u.w};
        } else if (t.mode == WG_RELU_BIAS) {
            v = f32x4{fmaxf(w.x + t.bias, 0.0f), fmaxf(w.y + t.bias, 0.0f), fmaxf(w.z + t.bias, 0.0f), fmaxf(w.w + t.bias, 0.0f)};
        }
        return v;
    }
    // an unaligned shift: plain rows only (h(p - d) with d = 1, 2, the Toeplitz rows)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = q + i >= 0 ? s[q + i] : 0.0f;
    return v;
}

__global__ __launch_bounds__(64) void k_wnb_wgrad(const WgradParams p) {
    const int lane = threadIdx.x, kl = lane >> 4, j = lane & 15;
    const int mb = blockIdx.x / p.kblocks, kb = blockIdx.x % p.kblocks, seg = blockIdx.y;
    const long long N = p.N;
    const int cpu = p.N / 16;  // chunks per utterance
    WgLane ta[4], tb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ta[i] = wg_resolve(p.a, mb * 64 + i * 16 + j, N);
        tb[i] = wg_resolve(p.bop, kb * 64 + i * 16 + j, N);
    }
    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[m][k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int c1 = min(p.chunks, (seg + 1) * p.cps);
    for (int c = seg * p.cps; c < c1; ++c) {
        const long long b = c / cpu;
        const int pos = (c - (int)b * cpu) * 16 + 4 * kl;
        f32x4 av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            av[i] = wg_fetch(ta[i], b, pos);
            bv[i] = wg_fetch(tb[i], b, pos);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[m][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][i], bv[k][i], acc[m][k], 0, 0, 0);
    }
    const int KP = p.kblocks * 64, MP = p.mblocks * 64;
    float* out = p.part + ((long long)seg * MP + mb * 64) * KP + kb * 64;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m * 16 + 4 * kl + r;
#pragma unroll
            for (int k = 0; k < 4; ++k) out[(long long)row * KP + k * 16 + j] = acc[m][k][r];
        }
}

// where dW goes: rows split at `msplit` into two groups (filter | gate, res | skip), columns into up to three ranges (tap 0,
// tap 1, conditioning), each a strided view of a PyTorch tensor; every group's row sum goes to up to two biases
struct WgOut {
    int M, K, msplit, segs, MP, KP;
    int kend[3], kvalid[3], rs[3], cs[3];
    float* w[2][3];
    float* bias[2][2];
    const float* part;
};

__global__ __launch_bounds__(256) void k_wnb_reduce(const WgOut o) {
    const long long total = (long long)o.M * o.K;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int m = (int)(idx / o.K), k = (int)(idx % o.K);
        const int rg = m >= o.msplit, mm = m - rg * o.msplit;
        double a = 0.0;
        for (int s = 0; s < o.segs; ++s) a += (double)o.part[((long long)s * o.MP + m) * o.KP + k];
        int k0 = 0;
        for (int c = 0; c < 3; ++c) {
            if (k < o.kend[c]) {
                if (k - k0 < o.kvalid[c]) o.w[rg][c][(long long)mm * o.rs[c] + (long long)(k - k0) * o.cs[c]] = (float)a;
                break;
            }
            k0 = o.kend[c];
        }
    }
}

// the bias gradients: row blockIdx.x of A summed over all positions
__global__ __launch_bounds__(256) void k_wnb_rowsum(const WgSide a, const WgOut o, int B, int N) {
    __shared__ double red[256];
    const int m = blockIdx.x, rg = m >= o.msplit, mm = m - rg * o.msplit;
    const WgLane t = wg_resolve(a, m, N);
    const int words = N / 4;
    double acc = 0.0;
    for (long long w = threadIdx.x; w < (long long)B * words; w += 256) {
        const f32x4 v = wg_fetch(t, w / words, (int)(w % words) * 4);
        acc += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (o.bias[rg][0]) o.bias[rg][0][mm] = (float)red[0];
        if (o.bias[rg][1]) o.bias[rg][1][mm] = (float)red[0];
    }
}

}  // namespace fpc_wn

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

