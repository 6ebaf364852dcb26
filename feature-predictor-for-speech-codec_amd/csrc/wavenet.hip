// wavenet.hip -- the reference's own vocoder, the Gaussian-output WaveNet of src/models/wavenet.py, as a batched decoder
// (gfx950).  Host side: configuration check, weight packing, the frame-rate conditioning kernels and the launches; the
// sample loop is k_wn_decode (wavenet_decode.h), the time-parallel teacher-forced pass the k_wnf_* family (wavenet_forward.h),
// the loss and the backward pass the k_wnb_* family (wavenet_backward.h).
//
// Conditioning (wavenet.py:93-115) runs once per call in plain HIP, one thread per output value: k_wn_frame is the
// embedding + concatenation + Conv1d(3) / Linear + tanh at frame rate, k_wn_upsample one ConvTranspose2d(1,1,(3,2s)) +
// LeakyReLU(0.4) stage.  The transposed convolution is two-dimensional: three taps run across the channel axis, so channel
// ch of the output reads channels ch-1..ch+1 of the input, and every output time reads two input times.
#include "wavenet_backward.h"
#include <algorithm>
#include <new>

// packed fp32 code generation is off for this source too (wavenet_decode.h)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

using namespace fpc_wn;

struct fpc_wavenet {
    fpc_wavenet_config c;
    int nfeat = 0, coutp = 0, layers = 0;
    long long sumdil = 0;
    bool shape_only = true;
    int device = 0, cus = 0;
    fpc::DevBuf emb, cw0, cb0, cw1, cb1, fw0, fb0, fw1, fb1, up0, up1;
    float upb[2] = {0, 0};
    fpc::DevBuf w_front, b_front, w1, b1, w2, b_res, b_skip, w_f1, b_f1, w_f2, dil_d, off_d;
    float b_f2[2] = {0, 0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    int last_nu = 0;
    int tn = 0;  // positions per workgroup of the time-parallel pass: 16, 32, 64, or 0 = the widest that fits
    fpc::DevBuf w1t, w2t, w_f1t, f2;  // the backward pass's transposed A operands, and final2_w plain
    int btn = 0;                      // positions per workgroup of k_wnb_final / k_wnb_layer: 16, 32 or 0 = automatic
};

namespace {

constexpr size_t LDS_BYTES = 160 * 1024;  // gfx950

int round_up(int v, int m) { return (v + m - 1) / m * m; }

size_t lds_bytes(const fpc_wavenet_config& c, int coutp, int nu) {
    const int rowsA = std::max(2 * c.residual_channels + coutp, c.skip_channels);
    const int rowsZ = std::max(c.gate_channels, c.skip_channels);
    return (size_t)nu * (rowsA + rowsZ + c.inp_channels * FRONT + 16) * sizeof(float);  // + the 16 LPC taps
}

int validate(const fpc_wavenet_config* c) {
    FPC_REQUIRE(c != nullptr, "fpc_wavenet: null configuration");
    FPC_REQUIRE(c->out_channels == 2, "fpc_wavenet: out_channels = %d; only the Gaussian output (2) is built", c->out_channels);
    FPC_REQUIRE(c->kernel_size == 2, "fpc_wavenet: kernel_size = %d; only 2 is built", c->kernel_size);
    FPC_REQUIRE(c->causal != 0, "fpc_wavenet: non-causal models are not built");
    FPC_REQUIRE(c->local == 0, "fpc_wavenet: local=True (repeated features, no upsampling network) is not built");
    FPC_REQUIRE(c->fat_upsampler != 0, "fpc_wavenet: fat_upsampler=False is not built");
    FPC_REQUIRE(c->upsample_scales[0] == 10 && c->upsample_scales[1] == 16,
                "fpc_wavenet: upsample_scales = [%d, %d]; only [10, 16] is built", c->upsample_scales[0],
                c->upsample_scales[1]);
    FPC_REQUIRE(c->inp_channels == 1 || c->inp_channels == 3, "fpc_wavenet: inp_channels = %d, not 1 or 3", c->inp_channels);
    const int w[3] = {c->residual_channels, c->gate_channels, c->skip_channels};
    for (int v : w) FPC_REQUIRE(v >= 16 && v % 16 == 0, "fpc_wavenet: channel width %d is not a positive multiple of 16", v);
    const int nfeat = c->cin_channels - 64;
    FPC_REQUIRE(nfeat == 20 || nfeat == 36, "fpc_wavenet: cin_channels = %d; 64 + 20 or 64 + 36 expected", c->cin_channels);
    FPC_REQUIRE(c->cout_channels >= 1 && c->num_blocks >= 1 && c->num_layers >= 1, "fpc_wavenet: empty model");
    FPC_REQUIRE(c->nu == 0 || c->nu == 16 || c->nu == 32, "fpc_wavenet: nu = %d, not 0, 16 or 32", c->nu);
    const bool fits = w[0] <= 512 && w[1] <= 512 && w[2] <= 512 && c->cout_channels <= 512 && c->num_layers <= 10 &&
                      c->num_blocks <= 4096 &&
                      lds_bytes(*c, round_up(c->cout_channels, 16), c->nu ? c->nu : 16) <= LDS_BYTES;
    if (!fits) {
        fpc::set_error("fpc_wavenet: R/G/S/cout %d/%d/%d/%d, %d layers per block, nu %d exceed the kernel's layout (widths <= 512, "
                       "dilation <= 512, 160 KiB of LDS)", w[0], w[1], w[2], c->cout_channels, c->num_layers, c->nu);
        return FPC_ERR_CAPACITY;
    }
    return FPC_OK;
}

// A [16 Mtiles x 16 Kq] in the per-lane order of the MFMA A operand (wavenet_decode.h)
template <class F>
void pack_tile(std::vector<float>& dst, int Kq, F at /* (row in tile, k) */) {
    for (int q = 0; q < Kq; ++q)
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 4; ++i) dst.push_back(at(l % 16, q * 16 + i * 4 + l / 16));
}

// one value per thread: out[b,t,co] = tanh(bias[co] + sum_{k,ci} w[co,ci,k] in[b, t - taps/2 + k, ci]); the first cin_in
// channels come from `in` [B,T,cin_in], the rest (the first layer's 64) from the pitch embedding
__global__ __launch_bounds__(256) void k_wn_frame(const float* __restrict__ in, int cin_in, const int* __restrict__ periods,
                                                  const float* __restrict__ emb, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float* __restrict__ out, int B, int T,
                                                  int cin, int cout, int taps) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * T * cout) return;
    const int co = (int)(idx % cout), t = (int)(idx / cout % T);
    const long long b = idx / ((long long)cout * T);
    float acc = 0.0f;  // the bias last, as torch adds it
    for (int k = 0; k < taps; ++k) {
        const int tt = t - taps / 2 + k;
        if (tt < 0 || tt >= T) continue;
        const float* row = in + (b * T + tt) * cin_in;
        const float* e = nullptr;
        if (cin > cin_in) {
            int per = periods[b * T + tt];
            per = per < 0 ? 0 : per > 255 ? 255 : per;
            e = emb + per * 64;
        }
        const float* wk = w + (long long)co * cin * taps + k;
        for (int ci = 0; ci < cin; ++ci) acc = fmaf(wk[ci * taps], ci < cin_in ? row[ci] : e[ci - cin_in], acc);
    }
    out[idx] = tanh_e(acc + bias[co]);
}

// out[b,ch,tq] = leaky(bias + sum_{kh<3} sum_{ti} in[b, ch + 1 - kh, ti] w[kh, tq + s/2 - ti s]), 0 <= kw < 2s: ti = hi - 1, hi
// nu = 0: out is [B][C][Lout].  nu = 16 / 32: the decode kernel's layout [tile][tq][C][nu], utterance b = tile * nu + column, so
// that a sample step reads its C x nu conditioning values as one contiguous block; columns past B are written as zero.
__global__ __launch_bounds__(256) void k_wn_upsample(const float* __restrict__ in, long long sb, long long sc, long long st,
                                                     const float* __restrict__ w, float bias, int s, float* __restrict__ out,
                                                     int B, int C, int Lin, int nu) {
    const long long Lout = (long long)Lin * s, total = (nu ? (long long)(B + nu - 1) / nu * nu : B) * C * Lout;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        int tq, ch;
        long long b;
        if (nu) {
            ch = (int)(idx / nu % C), tq = (int)(idx / ((long long)nu * C) % Lout);
            b = idx / ((long long)nu * C * Lout) * nu + idx % nu;
            if (b >= B) {
                out[idx] = 0.0f;
                continue;
            }
        } else {
            tq = (int)(idx % Lout), ch = (int)(idx / Lout % C);
            b = idx / (Lout * C);
        }
        const int hi = (tq + s / 2) / s;
        float acc = 0.0f;
        for (int kh = 0; kh < 3; ++kh) {
            const int cc = ch + 1 - kh;
            if (cc < 0 || cc >= C) continue;
            for (int ti = hi - 1; ti <= hi; ++ti) {
                if (ti < 0 || ti >= Lin) continue;
                acc = fmaf(in[b * sb + cc * sc + ti * st], w[kh * 2 * s + tq + s / 2 - ti * s], acc);
            }
        }
        acc = acc + bias;
        out[idx] = acc > 0.0f ? acc : 0.4f * acc;
    }
}

struct Workspace {
    float *cfeat, *fa, *fb, *u1, *ring;
};
long long ws_floats(const fpc_wavenet* m, long long B, long long T, Workspace* w, float* base) {
    const long long cf = (B + 31) / 32 * 32 * m->c.cout_channels * 160 * T, fr = B * T * m->c.cout_channels;
    const long long q = (B + 31) / 32 * 32 * m->c.residual_channels * m->sumdil;
    if (w) {
        w->cfeat = base;
        w->fa = base + cf;
        w->fb = w->fa + fr;
        w->u1 = w->fb + fr;
        w->ring = w->u1 + 10 * fr;
    }
    return cf + 12 * fr + q;
}

int check_call(const fpc_wavenet* m, int B, int T, const void* ws) {
    FPC_REQUIRE(m != nullptr, "fpc_wavenet: null handle");
    FPC_REQUIRE(!m->shape_only, "fpc_wavenet: the handle was created without weights (sizes only)");
    FPC_REQUIRE(B >= 1 && T >= 1 && (long long)T * 160 < (1ll << 31), "fpc_wavenet: B = %d, T = %d", B, T);
    FPC_REQUIRE(ws != nullptr && ((uintptr_t)ws & 15) == 0, "fpc_wavenet: the workspace must be a 16-byte aligned device block");
    return FPC_OK;
}

int pick_nu(const fpc_wavenet* m, int B) {
    if (m->c.nu) return m->c.nu;
    // one tile of 16 per compute unit while the batch allows it; beyond that two N tiles share each weight fragment
    const bool fits32 = lds_bytes(m->c, m->coutp, 32) <= LDS_BYTES;
    return (fits32 && B > 16 * m->cus) ? 32 : 16;
}

int run_condition(fpc_wavenet* m, const float* feat, const int* periods, int B, int T, float* cfeat, int nu,
                  const Workspace& w, hipStream_t st) {
    const int cout = m->c.cout_channels, cin = m->c.cin_channels;
    const long long nfr = (long long)B * T * cout;
    const unsigned gfr = (unsigned)((nfr + 255) / 256);
    k_wn_frame<<<gfr, 256, 0, st>>>(feat, m->nfeat, periods, m->emb.as<float>(), m->cw0.as<float>(), m->cb0.as<float>(), w.fa,
                                    B, T, cin, cout, 3);
    k_wn_frame<<<gfr, 256, 0, st>>>(w.fa, cout, nullptr, nullptr, m->cw1.as<float>(), m->cb1.as<float>(), w.fb, B, T, cout,
                                    cout, 3);
    k_wn_frame<<<gfr, 256, 0, st>>>(w.fb, cout, nullptr, nullptr, m->fw0.as<float>(), m->fb0.as<float>(), w.fa, B, T, cout,
                                    cout, 1);
    k_wn_frame<<<gfr, 256, 0, st>>>(w.fa, cout, nullptr, nullptr, m->fw1.as<float>(), m->fb1.as<float>(), w.fb, B, T, cout,
                                    cout, 1);
    const auto grid = [](long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 1 << 20); };
    // stage 1 reads the frame-rate result [B,T,cout] as [B,cout,T]
    k_wn_upsample<<<grid(nfr * 10), 256, 0, st>>>(w.fb, (long long)T * cout, 1, cout, m->up0.as<float>(), m->upb[0], 10, w.u1, B,
                                                  cout, T, 0);
    k_wn_upsample<<<grid((long long)(B + 31) / 32 * 32 * T * cout * 160), 256, 0, st>>>(w.u1, (long long)cout * T * 10, (long long)T * 10, 1, m->up1.as<float>(),
                                                   m->upb[1], 16, cfeat, B, cout, T * 10, nu);
    FPC_HIP(hipGetLastError());
    return FPC_OK;
}

int run_decode(fpc_wavenet* m, int B, int T, const Workspace& w, const float* lpc, const unsigned long long* seeds,
               const float* noise, const float* xin, float* out, float* xout, float* stats, hipStream_t st) {
    const fpc_wavenet_config& c = m->c;
    const int nu = pick_nu(m, B);
    DecodeParams p{};
    p.B = B;
    p.T = T;
    p.N = T * 160;
    p.R = c.residual_channels;
    p.G = c.gate_channels;
    p.S = c.skip_channels;
    p.cout = c.cout_channels;
    p.coutp = m->coutp;
    p.inp = c.inp_channels;
    p.layers = m->layers;
    p.K0q = c.inp_channels * FRONT / 16;
    p.K1q = (2 * p.R + p.coutp) / 16;
    p.Gq = p.G / 16;
    p.Sq = p.S / 16;
    p.rowsA = std::max(2 * p.R + p.coutp, p.S);
    p.rowsZ = std::max(p.G, p.S);
    p.w_front = m->w_front.as<float4>();
    p.b_front = m->b_front.as<float>();
    p.w1 = m->w1.as<float4>();
    p.b1 = m->b1.as<float>();
    p.w2 = m->w2.as<float4>();
    p.b_res = m->b_res.as<float>();
    p.b_skip = m->b_skip.as<float>();
    p.w_f1 = m->w_f1.as<float4>();
    p.b_f1 = m->b_f1.as<float>();
    p.w_f2 = m->w_f2.as<float4>();
    p.b_f2[0] = m->b_f2[0];
    p.b_f2[1] = m->b_f2[1];
    p.dil = m->dil_d.as<int>();
    p.ring_off = m->off_d.as<long long>();
    p.ring = w.ring;
    p.ring_cols = m->sumdil;
    p.cfeat = w.cfeat;
    p.lpc = lpc;
    p.seeds = seeds;
    p.noise = noise;
    p.xin = xin;
    p.out = out;
    p.xout = xout;
    p.stats = stats;
    const int tiles = (B + nu - 1) / nu;
    const long long ring4 = (long long)tiles * nu * p.R * m->sumdil / 4;
    const size_t lds = lds_bytes(c, m->coutp, nu);
    FPC_HIP(hipEventRecord(m->ev0, st));
    k_wn_clear<<<(unsigned)std::min<long long>((ring4 + 255) / 256, 4096), 256, 0, st>>>((float4*)w.ring, ring4);
    if (nu == 16) {
        FPC_HIP(hipFuncSetAttribute((const void*)k_wn_decode<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_wn_decode<16><<<tiles, THREADS, lds, st>>>(p);
    } else {
        FPC_HIP(hipFuncSetAttribute((const void*)k_wn_decode<32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_wn_decode<32><<<tiles, THREADS, lds, st>>>(p);
    }
    FPC_HIP(hipGetLastError());
    FPC_HIP(hipEventRecord(m->ev1, st));
    m->timed = true;
    m->last_nu = nu;
    return FPC_OK;
}

// ---- the time-parallel teacher-forced pass (wavenet_forward.h) ----

// LDS of the widest of the three MFMA kernels at TN positions: the layer's BA + Z panels, the last stage's Z + O, the
// front layer's inputs with their halo
size_t fwd_lds_bytes(const fpc_wavenet_config& c, int coutp, int tn) {
    const int rows = std::max(2 * c.residual_channels + coutp + c.gate_channels, 2 * c.skip_channels);
    return std::max((size_t)rows * tn, (size_t)c.inp_channels * (tn + FRONT)) * sizeof(float);
}

int pick_tn(const fpc_wavenet* m) {
    if (m->tn) return m->tn;
    // By measurement (profiles/wavenet_forward.txt): at the configured shape 32 makes 63.7 % of the MFMA peak and 64 makes
    // 58.8 %.  k_wnf_layer<32> stays within 64 VGPRs and 80 KiB, so two workgroups share a compute unit and one's staging and
    // gating run under the other's MFMAs; <64> fills the LDS alone.  So 64 is never the automatic choice.
    if (fwd_lds_bytes(m->c, m->coutp, 32) <= LDS_BYTES) return 32;
    return 16;  // every model `validate` admits fits at 16: (2 * 512 + 512 + 512) * 16 floats = 128 KiB
}

struct FwdWorkspace {
    Workspace c;  // cfeat [B][cout][N] and the conditioning's intermediates
    float *h[2], *skip, *inp;
};
long long fwd_floats(const fpc_wavenet* m, long long B, long long T, FwdWorkspace* w, float* base) {
    const long long N = 160 * T, cf = B * m->c.cout_channels * N, fr = B * T * m->c.cout_channels;
    const long long h = B * m->c.residual_channels * N, sk = B * m->c.skip_channels * N, in = B * m->c.inp_channels * N;
    if (w) {
        w->c.cfeat = base;
        w->c.fa = base + cf;
        w->c.fb = w->c.fa + fr;
        w->c.u1 = w->c.fb + fr;
        w->c.ring = nullptr;
        w->h[0] = w->c.u1 + 10 * fr;
        w->h[1] = w->h[0] + h;
        w->skip = w->h[1] + h;
        w->inp = w->skip + sk;
    }
    return cf + 12 * fr + 2 * h + sk + in;
}

// SAVE: the pass before a backward; hs = the layers' inputs, one [B][R][N] buffer each, ts = their t, s [B][2G][N] each
template <int TN, bool SAVE = false>
int launch_forward(const fpc_wavenet* m, ForwardParams p, const FwdWorkspace& w, hipStream_t st, float* hs = nullptr,
                   float* ts = nullptr) {
    const fpc_wavenet_config& c = m->c;
    const unsigned grid = (unsigned)((long long)p.B * p.tiles);
    const size_t lds_front = (size_t)p.inp * (TN + FRONT) * sizeof(float);
    const size_t lds_layer = (size_t)(2 * p.R + p.coutp + p.G) * TN * sizeof(float);
    const size_t lds_final = (size_t)2 * p.S * TN * sizeof(float);
    FPC_HIP(hipFuncSetAttribute((const void*)k_wnf_layer<TN, SAVE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_layer));
    FPC_HIP(hipFuncSetAttribute((const void*)k_wnf_final<TN, SAVE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_final));
    const long long hsz = (long long)p.B * p.R * p.N;
    p.hout = SAVE ? hs : w.h[0];
    k_wnf_front<TN><<<grid, THREADS, lds_front, st>>>(p);
    const float4 *w1 = p.w1, *w2 = p.w2;
    const float *b1 = p.b1, *b_res = p.b_res;
    for (int n = 0; n < m->layers; ++n) {
        p.w1 = w1 + (long long)n * (p.G / 16) * 2 * p.K1q * 64;
        p.b1 = b1 + (long long)n * 2 * p.G;
        p.w2 = w2 + (long long)n * ((p.R + p.S) / 16) * p.Gq * 64;
        p.b_res = b_res + (long long)n * p.R;
        p.dil = 1 << (n % c.num_layers);
        p.first = n == 0;
        p.last = n + 1 == m->layers;
        p.hin = SAVE ? hs + n * hsz : w.h[n & 1];
        p.hout = SAVE ? hs + (n + 1 < m->layers ? n + 1 : 0) * hsz : w.h[(n + 1) & 1];  // the last block stores no h
        if (SAVE) p.ts = ts + (long long)n * 2 * p.G * p.B * p.N;
        k_wnf_layer<TN, SAVE><<<grid, THREADS, lds_layer, st>>>(p);
    }
    k_wnf_final<TN, SAVE><<<grid, THREADS, lds_final, st>>>(p);
    FPC_HIP(hipGetLastError());
    return FPC_OK;
}

// the shape and weight members of the forward's parameters
int forward_params(const fpc_wavenet* m, int B, int T, int tn, ForwardParams& p) {
    const fpc_wavenet_config& c = m->c;
    p.B = B;
    p.T = T;
    p.N = T * 160;
    p.tiles = (p.N + tn - 1) / tn;
    if ((long long)B * p.tiles > 0x7fffffffll) {
        fpc::set_error("fpc_wavenet: B = %d, T = %d make more than 2^31 workgroups; chunked passes are not built", B, T);
        return FPC_ERR_CAPACITY;
    }
    p.R = c.residual_channels;
    p.G = c.gate_channels;
    p.S = c.skip_channels;
    p.cout = c.cout_channels;
    p.coutp = m->coutp;
    p.inp = c.inp_channels;
    p.K0q = c.inp_channels * FRONT / 16;
    p.K1q = (2 * p.R + p.coutp) / 16;
    p.Gq = p.G / 16;
    p.Sq = p.S / 16;
    p.w_front = m->w_front.as<float4>();
    p.b_front = m->b_front.as<float>();
    p.w1 = m->w1.as<float4>();
    p.b1 = m->b1.as<float>();
    p.w2 = m->w2.as<float4>();
    p.b_res = m->b_res.as<float>();
    p.b_skip = m->b_skip.as<float>();
    p.w_f1 = m->w_f1.as<float4>();
    p.b_f1 = m->b_f1.as<float>();
    p.w_f2 = m->w_f2.as<float4>();
    p.b_f2[0] = m->b_f2[0];
    p.b_f2[1] = m->b_f2[1];
    return FPC_OK;
}

// x != null: the input channels are built from x and the LPC taps into the workspace; else `inp` holds the caller's own
int run_forward(fpc_wavenet* m, const float* feat, const int* periods, const float* lpc, const float* x, const float* inp, int B,
                int T, float* stats, void* workspace, hipStream_t st) {
    const int tn = pick_tn(m);
    ForwardParams p{};
    const int rc0 = forward_params(m, B, T, tn, p);
    if (rc0 != FPC_OK) return rc0;
    FwdWorkspace w;
    fwd_floats(m, B, T, &w, static_cast<float*>(workspace));
    const int rc = run_condition(m, feat, periods, B, T, w.c.cfeat, 0, w.c, st);
    if (rc != FPC_OK) return rc;
    p.x = x;
    p.lpc = lpc;
    p.inp_out = w.inp;
    p.inp_in = x ? w.inp : inp;
    p.cfeat = w.c.cfeat;
    p.skip = w.skip;
    p.stats = stats;
    if (x) k_wnf_inputs<<<(unsigned)std::min<long long>(((long long)B * p.N + 255) / 256, 1 << 20), 256, 0, st>>>(p);
    return tn == 64 ? launch_forward<64>(m, p, w, st) : tn == 32 ? launch_forward<32>(m, p, w, st) : launch_forward<16>(m, p, w, st);
}

// ---- the loss and the backward pass (wavenet_backward.h) ----

constexpr int WG_SEGS = 32;  // position segments of a weight gradient at most
constexpr int WG_CPS = 2;    // 16-position chunks per segment at least: short float32 chains, the segments add in float64

size_t bwd_lds_bytes(const fpc_wavenet_config& c, int tn) {
    return (size_t)(c.residual_channels + c.skip_channels + 2 * c.gate_channels) * tn * sizeof(float);
}

int pick_btn(const fpc_wavenet* m) {
    if (m->btn) return m->btn;
    return bwd_lds_bytes(m->c, 32) <= LDS_BYTES ? 32 : 16;  // 16 fits every model `validate` admits: 2048 rows x 16 = 128 KiB
}

struct BwdWorkspace {
    Workspace c;
    float *hs, *ts, *skip, *osave, *stats, *dstats, *dskip, *do1, *da, *dhp, *dh[2], *e0[2], *part;
    double* lossb;
};
// the largest padded dW of the five weight-gradient products
long long wg_part_floats(const fpc_wavenet* m) {
    const fpc_wavenet_config& c = m->c;
    const auto up64 = [](long long v) { return (v + 63) / 64 * 64; };
    const long long R = c.residual_channels, G = c.gate_channels, S = c.skip_channels;
    const long long M[5] = {2 * G, R + S, R, S, 16}, K[5] = {2 * R + m->coutp, G, c.inp_channels * FRONT, S, S};
    long long mk = 0;
    for (int i = 0; i < 5; ++i) mk = std::max(mk, up64(M[i]) * up64(K[i]));
    return mk;
}
// B T [160 (cout + L R + L 2G + 4 S + 4 + 2G + 5 R) + 12 cout] + 2 B + WG_SEGS max M K
long long bwd_floats(const fpc_wavenet* m, long long B, long long T, BwdWorkspace* w, float* base) {
    const long long N = 160 * T, cf = B * m->c.cout_channels * N, fr = B * T * m->c.cout_channels, L = m->layers;
    const long long h = B * m->c.residual_channels * N, sk = B * m->c.skip_channels * N, g2 = 2 * B * m->c.gate_channels * N;
    const long long mk = wg_part_floats(m);
    if (w) {
        float* q = base;
        const auto take = [&](long long n) {
            float* r = q;
            q += n;
            return r;
        };
        w->c.cfeat = take(cf);
        w->c.fa = take(fr);
        w->c.fb = take(fr);
        w->c.u1 = take(10 * fr);
        w->c.ring = nullptr;
        w->hs = take(L * h);
        w->ts = take(L * g2);
        w->skip = take(sk);
        w->osave = take(sk);
        w->dskip = take(sk);
        w->do1 = take(sk);
        w->stats = take(2 * B * N);
        w->dstats = take(2 * B * N);
        w->da = take(g2);
        w->dhp = take(h);
        w->dh[0] = take(h);
        w->dh[1] = take(h);
        w->e0[0] = take(h);
        w->e0[1] = take(h);
        w->part = take(WG_SEGS * mk);
        w->lossb = reinterpret_cast<double*>(take(2 * B));  // an even offset: every count above is even
    }
    return cf + 12 * fr + L * h + L * g2 + 4 * sk + 4 * B * N + g2 + 5 * h + WG_SEGS * mk + 2 * B;
}

WgRows wg_rows(const float* src, long long bstride, int rows, int valid, int shift = 0) {
    return WgRows{src, bstride, rows, valid, shift, 0, 1, WG_PLAIN, 0, nullptr};
}

// dW = sum_p A Bop^T over all B N positions, then the segments in order into the tensors `o` names
int run_wgrad(WgradParams p, WgOut o, int B, int N, const BwdWorkspace& w, hipStream_t st) {
    p.N = N;
    p.chunks = B * (N / 16);
    p.cps = std::max(WG_CPS, (p.chunks + WG_SEGS - 1) / WG_SEGS);
    const int segs = (p.chunks + p.cps - 1) / p.cps;
    p.mblocks = (p.a.total + 63) / 64;
    p.kblocks = (p.bop.total + 63) / 64;
    p.part = w.part;
    o.segs = segs;
    o.MP = p.mblocks * 64;
    o.KP = p.kblocks * 64;
    o.part = w.part;
    k_wnb_wgrad<<<dim3((unsigned)(p.mblocks * p.kblocks), (unsigned)segs), 64, 0, st>>>(p);
    k_wnb_reduce<<<(unsigned)(((long long)o.M * o.K + 255) / 256), 256, 0, st>>>(o);
    k_wnb_rowsum<<<o.M, 256, 0, st>>>(p.a, o, B, N);
    return FPC_OK;
}

template <int TN>
int launch_backward(const fpc_wavenet* m, BackwardParams p, const BwdWorkspace& w, const float* inp, const fpc_wavenet_grads& g,
                    hipStream_t st) {
    const fpc_wavenet_config& c = m->c;
    const int B = p.B, N = p.N, R = p.R, G = p.G, S = p.S, cout = p.cout, coutp = p.coutp, L = m->layers;
    p.tiles = (N + TN - 1) / TN;
    const unsigned grid = (unsigned)((long long)B * p.tiles);
    const size_t lds_layer = bwd_lds_bytes(c, TN), lds_final = (size_t)S * TN * sizeof(float);
    FPC_HIP(hipFuncSetAttribute((const void*)k_wnb_layer<TN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_layer));
    FPC_HIP(hipFuncSetAttribute((const void*)k_wnb_final<TN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_final));
    const long long hsz = (long long)B * R * N, gsz = 2ll * B * G * N;

    k_wnb_loss<<<B, 256, 0, st>>>(p);
    k_wnb_loss_sum<<<1, 1, 0, st>>>(p);
    k_wnb_final<TN><<<grid, THREADS, lds_final, st>>>(p);
    {   // final_conv.3: dstats . o^T;  final_conv.1: do1 . relu(skip + b_skip)^T
        WgradParams q{};
        q.a.g[0] = wg_rows(w.dstats, 2ll * N, 16, 2);
        q.a.total = 16;
        q.bop.g[0] = wg_rows(w.osave, (long long)S * N, S, S);
        q.bop.total = S;
        WgOut o{};
        o.M = 2, o.K = S, o.msplit = 2, o.kend[0] = o.kvalid[0] = S, o.rs[0] = S, o.cs[0] = 1;
        o.w[0][0] = g.final2_w, o.bias[0][0] = g.final2_b;
        run_wgrad(q, o, B, N, w, st);
        q.a.g[0] = wg_rows(w.do1, (long long)S * N, S, S);
        q.a.total = S;
        q.bop.g[0] = wg_rows(w.skip, (long long)S * N, S, S);
        q.bop.g[0].mode = WG_RELU_BIAS;
        q.bop.g[0].bias = m->b_skip.as<float>();
        o.M = S, o.msplit = S;
        o.w[0][0] = g.final1_w, o.bias[0][0] = g.final1_b;
        run_wgrad(q, o, B, N, w, st);
    }
    const int K1 = 2 * R + coutp;
    for (int n = L - 1; n >= 0; --n) {
        const int d = 1 << (n % c.num_layers), k = (L - 1 - n) & 1;  // this launch writes dh[k], e0[k] and reads [k ^ 1]
        p.w2t = m->w2t.as<float4>() + (long long)n * (G / 16) * p.K2q * 64;
        p.w1t = m->w1t.as<float4>() + (long long)n * (K1 / 16) * p.K1q * 64;
        p.ts = w.ts + n * gsz;
        p.last = p.first = n == L - 1;
        p.dil_next = n + 1 < L ? 1 << ((n + 1) % c.num_layers) : 0;
        p.dh_in = w.dh[k ^ 1];
        p.e0_in = w.e0[k ^ 1];
        p.dh_out = w.dh[k];
        p.e0_out = w.e0[k];
        k_wnb_layer<TN><<<grid, THREADS, lds_layer, st>>>(p);
        const float* hn = w.hs + n * hsz;
        WgradParams q{};  // dW1 = da . [h(p - d); h(p); c(p)]^T
        q.a.g[0] = wg_rows(w.da, 2ll * G * N, 2 * G, 2 * G);
        q.a.total = 2 * G;
        q.bop.g[0] = wg_rows(hn, (long long)R * N, R, R, d);
        q.bop.g[1] = wg_rows(hn, (long long)R * N, R, R);
        q.bop.g[2] = wg_rows(w.c.cfeat, (long long)cout * N, coutp, cout);
        q.bop.total = K1;
        WgOut o{};
        o.M = 2 * G, o.K = K1, o.msplit = G;
        o.kend[0] = R, o.kend[1] = 2 * R, o.kend[2] = K1;
        o.kvalid[0] = o.kvalid[1] = R, o.kvalid[2] = cout;
        o.rs[0] = o.rs[1] = 2 * R, o.cs[0] = o.cs[1] = 2, o.rs[2] = cout, o.cs[2] = 1;
        const long long wo = (long long)n * G * R * 2, co = (long long)n * G * cout, bo = (long long)n * G;
        o.w[0][0] = g.filter_w + wo, o.w[0][1] = g.filter_w + wo + 1, o.w[0][2] = g.filter_c_w + co;
        o.w[1][0] = g.gate_w + wo, o.w[1][1] = g.gate_w + wo + 1, o.w[1][2] = g.gate_c_w + co;
        o.bias[0][0] = g.filter_b + bo, o.bias[0][1] = g.filter_c_b + bo;
        o.bias[1][0] = g.gate_b + bo, o.bias[1][1] = g.gate_c_b + bo;
        run_wgrad(q, o, B, N, w, st);
        q = WgradParams{};  // dW2 = [sqrt(1/2) dh'; dskip] . (t s)^T
        q.a.g[0] = wg_rows(w.dhp, (long long)R * N, R, R);
        q.a.g[1] = wg_rows(w.dskip, (long long)S * N, S, S);
        q.a.total = R + S;
        q.bop.g[0] = wg_rows(p.ts, 2ll * G * N, G, G);
        q.bop.g[0].mode = WG_PRODUCT;
        q.bop.g[0].aux_off = (long long)G * N;
        q.bop.total = G;
        o = WgOut{};
        o.M = R + S, o.K = G, o.msplit = R, o.kend[0] = o.kvalid[0] = G, o.rs[0] = G, o.cs[0] = 1;
        o.w[0][0] = g.res_w + (long long)n * R * G, o.w[1][0] = g.skip_w + (long long)n * S * G;
        o.bias[0][0] = g.res_b + (long long)n * R, o.bias[1][0] = g.skip_b + (long long)n * S;
        run_wgrad(q, o, B, N, w, st);
    }
    // the front convolution: the first block wrote dh[(L - 1) & 1]; dpre0 takes dhp's place
    p.dh_in = w.dh[(L - 1) & 1];
    p.e0_in = w.e0[(L - 1) & 1];
    p.dil_next = 1;
    p.h0 = w.hs;
    p.dpre0 = w.dhp;
    k_wnb_front<<<(unsigned)std::min<long long>((hsz + 255) / 256, 1 << 20), 256, 0, st>>>(p);
    WgradParams q{};
    q.a.g[0] = wg_rows(w.dhp, (long long)R * N, R, R);
    q.a.total = R;
    q.bop.g[0] = WgRows{inp, (long long)c.inp_channels * N, c.inp_channels * FRONT, c.inp_channels * FRONT, FRONT - 1, -1, FRONT,
                        WG_PLAIN, 0, nullptr};
    q.bop.total = c.inp_channels * FRONT;
    WgOut o{};
    o.M = R, o.K = c.inp_channels * FRONT, o.msplit = R, o.kend[0] = o.kvalid[0] = o.K, o.rs[0] = o.K, o.cs[0] = 1;
    o.w[0][0] = g.front_w, o.bias[0][0] = g.front_b;
    run_wgrad(q, o, B, N, w, st);
    FPC_HIP(hipGetLastError());
    return FPC_OK;
}

int run_loss_backward(fpc_wavenet* m, const float* feat, const int* periods, const float* inp, const float* target, int n_valid,
                      int B, int T, float* loss, const fpc_wavenet_grads& g, void* workspace, hipStream_t st) {
    const int tn = pick_tn(m), btn = pick_btn(m);
    ForwardParams f{};
    const int rc0 = forward_params(m, B, T, std::min(tn, 16), f);  // 16: the bound on the grid covers every instance
    if (rc0 != FPC_OK) return rc0;
    f.tiles = (f.N + tn - 1) / tn;
    BwdWorkspace w;
    bwd_floats(m, B, T, &w, static_cast<float*>(workspace));
    const int rc = run_condition(m, feat, periods, B, T, w.c.cfeat, 0, w.c, st);
    if (rc != FPC_OK) return rc;
    FwdWorkspace fw{};
    fw.c = w.c;
    fw.skip = w.skip;
    f.inp_in = inp;
    f.cfeat = w.c.cfeat;
    f.skip = w.skip;
    f.stats = w.stats;
    f.osave = w.osave;
    const int rc1 = tn == 64   ? launch_forward<64, true>(m, f, fw, st, w.hs, w.ts)
                    : tn == 32 ? launch_forward<32, true>(m, f, fw, st, w.hs, w.ts)
                               : launch_forward<16, true>(m, f, fw, st, w.hs, w.ts);
    if (rc1 != FPC_OK) return rc1;
    BackwardParams p{};
    p.B = B;
    p.N = f.N;
    p.R = f.R, p.G = f.G, p.S = f.S, p.cout = f.cout, p.coutp = f.coutp;
    p.K2q = (p.R + p.S) / 16;
    p.K1q = 2 * p.G / 16;
    p.Sq = p.S / 16;
    p.n_valid = n_valid;
    p.inv_m = 1.0 / ((double)B * n_valid);
    p.stats = w.stats;
    p.target = target;
    p.dstats = w.dstats;
    p.lossb = w.lossb;
    p.loss = loss;
    p.f2 = m->f2.as<float>();
    p.w_f1t = m->w_f1t.as<float4>();
    p.osave = w.osave;
    p.skip = w.skip;
    p.b_skip = m->b_skip.as<float>();
    p.do1 = w.do1;
    p.dskip = w.dskip;
    p.dhp = w.dhp;
    p.da = w.da;
    p.dc = g.cfeat;
    return btn == 32 ? launch_backward<32>(m, p, w, inp, g, st) : launch_backward<16>(m, p, w, inp, g, st);
}

}  // namespace

extern "C" void fpc_wavenet_destroy(fpc_wavenet* m) {
    if (!m) return;
    if (m->ev0) (void)hipEventDestroy(m->ev0);
    if (m->ev1) (void)hipEventDestroy(m->ev1);
    delete m;
}

extern "C" int fpc_wavenet_create(const fpc_wavenet_config* cfg, const fpc_wavenet_weights* w, fpc_wavenet** out) {
    FPC_REQUIRE(out != nullptr, "fpc_wavenet_create: null output");
    *out = nullptr;
    const int rc = validate(cfg);
    if (rc != FPC_OK) return rc;
    fpc_wavenet* m = new (std::nothrow) fpc_wavenet;
    FPC_REQUIRE(m != nullptr, "fpc_wavenet_create: out of host memory");
    struct Guard {
        fpc_wavenet* m;
        ~Guard() { fpc_wavenet_destroy(m); }
    } guard{m};
    m->c = *cfg;
    m->nfeat = cfg->cin_channels - 64;
    m->coutp = round_up(cfg->cout_channels, 16);
    m->layers = cfg->num_blocks * cfg->num_layers;
    std::vector<int> dil(m->layers);
    std::vector<long long> off(m->layers);
    for (int n = 0; n < m->layers; ++n) {
        dil[n] = 1 << (n % cfg->num_layers);
        off[n] = m->sumdil;
        m->sumdil += dil[n];
    }
    if (w == nullptr) {  // sizes only: needs no device
        guard.m = nullptr;
        *out = m;
        return FPC_OK;
    }
    if (!fpc::have_device()) {
        fpc::set_error("fpc_wavenet_create: no HIP device");
        return FPC_ERR_NO_DEVICE;
    }
    const float* const* wp = reinterpret_cast<const float* const*>(w);
    for (size_t i = 0; i < sizeof(*w) / sizeof(float*); ++i) FPC_REQUIRE(wp[i] != nullptr, "fpc_wavenet_create: weight %zu is null", i);
    FPC_HIP(hipGetDevice(&m->device));
    FPC_HIP(hipDeviceGetAttribute(&m->cus, hipDeviceAttributeMultiprocessorCount, m->device));

    const int R = cfg->residual_channels, G = cfg->gate_channels, S = cfg->skip_channels, cout = cfg->cout_channels;
    const int cin = cfg->cin_channels, inp = cfg->inp_channels, L = m->layers, coutp = m->coutp;
    const auto up = [](fpc::DevBuf& d, const float* src, size_t n) {
        return d.upload(std::vector<float>(src, src + n));
    };
    FPC_HIP(up(m->emb, w->embedding, 256 * 64));
    FPC_HIP(up(m->cw0, w->c_conv0_w, (size_t)cout * cin * 3));
    FPC_HIP(up(m->cb0, w->c_conv0_b, cout));
    FPC_HIP(up(m->cw1, w->c_conv1_w, (size_t)cout * cout * 3));
    FPC_HIP(up(m->cb1, w->c_conv1_b, cout));
    FPC_HIP(up(m->fw0, w->c_fc0_w, (size_t)cout * cout));
    FPC_HIP(up(m->fb0, w->c_fc0_b, cout));
    FPC_HIP(up(m->fw1, w->c_fc1_w, (size_t)cout * cout));
    FPC_HIP(up(m->fb1, w->c_fc1_b, cout));
    FPC_HIP(up(m->up0, w->up0_w, 3 * 20));
    FPC_HIP(up(m->up1, w->up1_w, 3 * 32));
    m->upb[0] = w->up0_b[0];
    m->upb[1] = w->up1_b[0];

    std::vector<float> v;
    const int K0 = inp * FRONT, K1 = 2 * R + coutp;
    for (int t = 0; t < R / 16; ++t)  // K index = channel * 32 + tap
        pack_tile(v, K0 / 16, [&](int r, int k) { return w->front_w[(size_t)(t * 16 + r) * K0 + k]; });
    FPC_HIP(m->w_front.upload(v));
    FPC_HIP(up(m->b_front, w->front_b, R));

    v.clear();
    std::vector<float> b1((size_t)L * 2 * G);
    for (int n = 0; n < L; ++n)
        for (int t = 0; t < G / 16; ++t)
            for (int fg = 0; fg < 2; ++fg) {
                const float* cw = (fg ? w->gate_w : w->filter_w) + (size_t)n * G * R * 2;    // [G][R][2]
                const float* cc = (fg ? w->gate_c_w : w->filter_c_w) + (size_t)n * G * cout;  // [G][cout]
                pack_tile(v, K1 / 16, [&](int r, int k) {
                    const size_t g = t * 16 + r;
                    if (k < R) return cw[(g * R + k) * 2];                // tap 0: h(p - dil)
                    if (k < 2 * R) return cw[(g * R + (k - R)) * 2 + 1];  // tap 1: h(p)
                    return k - 2 * R < cout ? cc[g * cout + (k - 2 * R)] : 0.0f;
                });
            }
    for (int n = 0; n < L; ++n)
        for (int g = 0; g < G; ++g) {
            b1[((size_t)n * 2) * G + g] = w->filter_b[(size_t)n * G + g] + w->filter_c_b[(size_t)n * G + g];
            b1[((size_t)n * 2 + 1) * G + g] = w->gate_b[(size_t)n * G + g] + w->gate_c_b[(size_t)n * G + g];
        }
    FPC_HIP(m->w1.upload(v));
    FPC_HIP(m->b1.upload(b1));

    v.clear();
    for (int n = 0; n < L; ++n)
        for (int t = 0; t < (R + S) / 16; ++t)
            pack_tile(v, G / 16, [&](int r, int k) {
                const int row = t * 16 + r;
                return row < R ? w->res_w[((size_t)n * R + row) * G + k] : w->skip_w[((size_t)n * S + row - R) * G + k];
            });
    FPC_HIP(m->w2.upload(v));
    FPC_HIP(up(m->b_res, w->res_b, (size_t)L * R));
    std::vector<float> bs(S);
    for (int s = 0; s < S; ++s) {
        double a = 0.0;
        for (int n = 0; n < L; ++n) a += w->skip_b[(size_t)n * S + s];
        bs[s] = (float)a;
    }
    FPC_HIP(m->b_skip.upload(bs));

    v.clear();
    for (int t = 0; t < S / 16; ++t) pack_tile(v, S / 16, [&](int r, int k) { return w->final1_w[(size_t)(t * 16 + r) * S + k]; });
    FPC_HIP(m->w_f1.upload(v));
    FPC_HIP(up(m->b_f1, w->final1_b, S));
    v.clear();
    pack_tile(v, S / 16, [&](int r, int k) { return r < 2 ? w->final2_w[(size_t)r * S + k] : 0.0f; });
    FPC_HIP(m->w_f2.upload(v));
    m->b_f2[0] = w->final2_b[0];
    m->b_f2[1] = w->final2_b[1];

    // the backward pass's A operands (wavenet_backward.h): the same matrices transposed, in the same fragment order
    const auto w1_at = [&](int n, int row, int k) {  // [2G x K1] of layer n as packed above
        const int fg = row >= G, g = row - fg * G;
        const float* cw = (fg ? w->gate_w : w->filter_w) + (size_t)n * G * R * 2;
        const float* cc = (fg ? w->gate_c_w : w->filter_c_w) + (size_t)n * G * cout;
        if (k < R) return cw[((size_t)g * R + k) * 2];
        if (k < 2 * R) return cw[((size_t)g * R + (k - R)) * 2 + 1];
        return k - 2 * R < cout ? cc[(size_t)g * cout + (k - 2 * R)] : 0.0f;
    };
    v.clear();
    for (int n = 0; n < L; ++n)
        for (int t = 0; t < K1 / 16; ++t) pack_tile(v, 2 * G / 16, [&](int r, int k) { return w1_at(n, k, t * 16 + r); });
    FPC_HIP(m->w1t.upload(v));
    v.clear();
    for (int n = 0; n < L; ++n)
        for (int t = 0; t < G / 16; ++t)
            pack_tile(v, (R + S) / 16, [&](int r, int k) {
                const size_t g = t * 16 + r;
                return k < R ? w->res_w[((size_t)n * R + k) * G + g] : w->skip_w[((size_t)n * S + k - R) * G + g];
            });
    FPC_HIP(m->w2t.upload(v));
    v.clear();
    for (int t = 0; t < S / 16; ++t) pack_tile(v, S / 16, [&](int r, int k) { return w->final1_w[(size_t)k * S + t * 16 + r]; });
    FPC_HIP(m->w_f1t.upload(v));
    FPC_HIP(up(m->f2, w->final2_w, (size_t)2 * S));
    FPC_HIP(m->dil_d.upload(dil));
    FPC_HIP(m->off_d.upload(off));
    FPC_HIP(hipEventCreate(&m->ev0));
    FPC_HIP(hipEventCreate(&m->ev1));
    m->shape_only = false;
    guard.m = nullptr;
    *out = m;
    return FPC_OK;
}

extern "C" long long fpc_wavenet_workspace_bytes(const fpc_wavenet* m, int B, int T) {
    if (!m || B < 1 || T < 1) {
        fpc::set_error("fpc_wavenet_workspace_bytes: null handle or B, T < 1");
        return FPC_ERR_INVALID;
    }
    return 4 * ws_floats(m, B, T, nullptr, nullptr);
}

extern "C" int fpc_wavenet_condition(fpc_wavenet* m, const float* feat_dev, const int32_t* periods_dev, int B, int T,
                                     float* cfeat_dev, void* workspace_dev, fpc_stream s) {
    const int rc = check_call(m, B, T, workspace_dev);
    if (rc != FPC_OK) return rc;
    FPC_REQUIRE(feat_dev && periods_dev && cfeat_dev, "fpc_wavenet_condition: null pointer");
    Workspace w;
    ws_floats(m, B, T, &w, static_cast<float*>(workspace_dev));
    return run_condition(m, feat_dev, periods_dev, B, T, cfeat_dev, 0, w, static_cast<hipStream_t>(s));
}

extern "C" int fpc_wavenet_synthesize(fpc_wavenet* m, const float* feat_dev, const int32_t* periods_dev, const float* lpc_dev,
                                      int B, int T, const uint64_t* seeds_dev, const float* noise_dev, float* out_dev,
                                      float* x_dev, void* workspace_dev, fpc_stream s) {
    const int rc = check_call(m, B, T, workspace_dev);
    if (rc != FPC_OK) return rc;
    FPC_REQUIRE(feat_dev && periods_dev && lpc_dev && out_dev, "fpc_wavenet_synthesize: null pointer");
    FPC_REQUIRE(seeds_dev || noise_dev, "fpc_wavenet_synthesize: neither seeds nor noise");
    Workspace w;
    ws_floats(m, B, T, &w, static_cast<float*>(workspace_dev));
    const hipStream_t st = static_cast<hipStream_t>(s);
    const int rc2 = run_condition(m, feat_dev, periods_dev, B, T, w.cfeat, pick_nu(m, B), w, st);
    if (rc2 != FPC_OK) return rc2;
    return run_decode(m, B, T, w, lpc_dev, reinterpret_cast<const unsigned long long*>(seeds_dev), noise_dev, nullptr, out_dev,
                      x_dev, nullptr, st);
}

extern "C" int fpc_wavenet_forward(fpc_wavenet* m, const float* feat_dev, const int32_t* periods_dev, const float* lpc_dev,
                                   int B, int T, const float* x_dev, float* stats_dev, void* workspace_dev, fpc_stream s) {
    const int rc = check_call(m, B, T, workspace_dev);
    if (rc != FPC_OK) return rc;
    FPC_REQUIRE(feat_dev && periods_dev && lpc_dev && x_dev && stats_dev, "fpc_wavenet_forward: null pointer");
    Workspace w;
    ws_floats(m, B, T, &w, static_cast<float*>(workspace_dev));
    const hipStream_t st = static_cast<hipStream_t>(s);
    const int rc2 = run_condition(m, feat_dev, periods_dev, B, T, w.cfeat, pick_nu(m, B), w, st);
    if (rc2 != FPC_OK) return rc2;
    return run_decode(m, B, T, w, lpc_dev, nullptr, nullptr, x_dev, nullptr, nullptr, stats_dev, st);
}

extern "C" long long fpc_wavenet_forward_workspace_bytes(const fpc_wavenet* m, int B, int T) {
    if (!m || B < 1 || T < 1) {
        fpc::set_error("fpc_wavenet_forward_workspace_bytes: null handle or B, T < 1");
        return FPC_ERR_INVALID;
    }
    return 4 * fwd_floats(m, B, T, nullptr, nullptr);
}

extern "C" int fpc_wavenet_set_forward_tile(fpc_wavenet* m, int tn) {
    FPC_REQUIRE(m != nullptr, "fpc_wavenet_set_forward_tile: null handle");
    FPC_REQUIRE(tn == 0 || tn == 16 || tn == 32 || tn == 64, "fpc_wavenet_set_forward_tile: tn = %d, not 0, 16, 32 or 64", tn);
    if (tn && fwd_lds_bytes(m->c, m->coutp, tn) > LDS_BYTES) {
        fpc::set_error("fpc_wavenet_set_forward_tile: tn = %d needs %zu bytes of LDS for this model, the device has %zu", tn,
                       fwd_lds_bytes(m->c, m->coutp, tn), LDS_BYTES);
        return FPC_ERR_CAPACITY;
    }
    m->tn = tn;
    return FPC_OK;
}

extern "C" int fpc_wavenet_forward_tile(const fpc_wavenet* m) { return m ? pick_tn(m) : (int)FPC_ERR_INVALID; }

extern "C" int fpc_wavenet_forward_parallel(fpc_wavenet* m, const float* feat_dev, const int32_t* periods_dev,
                                            const float* lpc_dev, int B, int T, const float* x_dev, float* stats_dev,
                                            void* workspace_dev, fpc_stream s) {
    const int rc = check_call(m, B, T, workspace_dev);
    if (rc != FPC_OK) return rc;
    FPC_REQUIRE(feat_dev && periods_dev && lpc_dev && x_dev && stats_dev, "fpc_wavenet_forward_parallel: null pointer");
    return run_forward(m, feat_dev, periods_dev, lpc_dev, x_dev, nullptr, B, T, stats_dev, workspace_dev,
                       static_cast<hipStream_t>(s));
}

extern "C" int fpc_wavenet_forward_input(fpc_wavenet* m, const float* feat_dev, const int32_t* periods_dev, const float* inp_dev,
                                         int B, int T, float* stats_dev, void* workspace_dev, fpc_stream s) {
    const int rc = check_call(m, B, T, workspace_dev);
    if (rc != FPC_OK) return rc;
    FPC_REQUIRE(feat_dev && periods_dev && inp_dev && stats_dev, "fpc_wavenet_forward_input: null pointer");
    return run_forward(m, feat_dev, periods_dev, nullptr, nullptr, inp_dev, B, T, stats_dev, workspace_dev,
                       static_cast<hipStream_t>(s));
}

extern "C" long long fpc_wavenet_backward_workspace_bytes(const fpc_wavenet* m, int B, int T) {
    if (!m || B < 1 || T < 1) {
        fpc::set_error("fpc_wavenet_backward_workspace_bytes: null handle or B, T < 1");
        return FPC_ERR_INVALID;
    }
    return 4 * bwd_floats(m, B, T, nullptr, nullptr);
}

extern "C" long long fpc_wavenet_backward_stats_offset(const fpc_wavenet* m, int B, int T) {
    if (!m || B < 1 || T < 1) {
        fpc::set_error("fpc_wavenet_backward_stats_offset: null handle or B, T < 1");
        return FPC_ERR_INVALID;
    }
    BwdWorkspace w;
    bwd_floats(m, B, T, &w, nullptr);
    return (long long)reinterpret_cast<uintptr_t>(w.stats);
}

extern "C" int fpc_wavenet_set_backward_tile(fpc_wavenet* m, int tn) {
    FPC_REQUIRE(m != nullptr, "fpc_wavenet_set_backward_tile: null handle");
    FPC_REQUIRE(tn == 0 || tn == 16 || tn == 32, "fpc_wavenet_set_backward_tile: tn = %d, not 0, 16 or 32", tn);
    if (tn && bwd_lds_bytes(m->c, tn) > LDS_BYTES) {
        fpc::set_error("fpc_wavenet_set_backward_tile: tn = %d needs %zu bytes of LDS for this model, the device has %zu", tn,
                       bwd_lds_bytes(m->c, tn), LDS_BYTES);
        return FPC_ERR_CAPACITY;
    }
    m->btn = tn;
    return FPC_OK;
}

extern "C" int fpc_wavenet_backward_tile(const fpc_wavenet* m) { return m ? pick_btn(m) : (int)FPC_ERR_INVALID; }

extern "C" int fpc_wavenet_loss_backward(fpc_wavenet* m, const float* feat_dev, const int32_t* periods_dev, const float* inp_dev,
                                         const float* target_dev, int n_valid, int B, int T, float* loss_dev,
                                         const fpc_wavenet_grads* grads, void* workspace_dev, fpc_stream s) {
    FPC_REQUIRE(m != nullptr, "fpc_wavenet_loss_backward: null handle");
    FPC_REQUIRE(feat_dev && periods_dev && inp_dev && target_dev && loss_dev && grads, "fpc_wavenet_loss_backward: null pointer");
    FPC_REQUIRE(n_valid >= 1 && n_valid <= 160ll * T, "fpc_wavenet_loss_backward: n_valid = %d outside [1, 160 T], T = %d", n_valid, T);
    const int rc = check_call(m, B, T, workspace_dev);
    if (rc != FPC_OK) return rc;
    float* const* gp = reinterpret_cast<float* const*>(grads);
    for (size_t i = 0; i < sizeof(*grads) / sizeof(float*); ++i)
        FPC_REQUIRE(gp[i] != nullptr, "fpc_wavenet_loss_backward: gradient pointer %zu is null", i);
    FPC_REQUIRE(((uintptr_t)inp_dev & 15) == 0, "fpc_wavenet_loss_backward: inp must be 16-byte aligned");
    return run_loss_backward(m, feat_dev, periods_dev, inp_dev, target_dev, n_valid, B, T, loss_dev, *grads, workspace_dev,
                             static_cast<hipStream_t>(s));
}

extern "C" float fpc_wavenet_last_decode_ms(fpc_wavenet* m) {
    if (!m || !m->timed) return -1.0f;
    if (hipEventSynchronize(m->ev1) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, m->ev0, m->ev1) != hipSuccess) return -1.0f;
    return ms;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
