// bitstream.hip -- the codec's bitstream packed and unpacked on the device, a whole batch per launch (gfx950).
//
// Replaces the per-utterance, per-bit Python loops of fpcodec_amd/bitstream.py (pack / unpack, entropy_pack /
// entropy_unpack), which stay as the specification: the bytes here are theirs.  The symbols never leave the device: idx
// [B,L,4] is what fpc_encode writes and fpc_decode_features reads.
//
// Fixed-length framing -- the serial part is only WHERE a frame starts:
//   pack    one wavefront per utterance, one lane per frame, 64 frames per step.  A lane composes its frame (at most 2 + 16 +
//           32 bits) in a 64-bit word; an exclusive prefix sum of the widths over the wave (__shfl_up, no LDS) places it; the
//           lane ORs it into an LDS image of the step (ds_or_b32 on up to three dwords); the wave streams the finished
//           dwords out, coalesced, and carries the unfinished one into the next step.  No per-bit work.
//   unpack  the step's stretch of the row is staged in LDS; the two flag bits of a frame decide its length, so every lane
//           walks the same chain of 64 two-bit reads (broadcast LDS reads) and keeps the offset of its own frame; then one
//           lane per frame cuts its fields out of the image and writes one 16-byte idx row.
// Entropy-coded framing -- the chain through low / high is serial per stream, so the parallelism is across streams: one
// utterance per lane, 64-lane workgroups (a small batch still spreads over compute units), all cumulative tables in LDS,
// the renormalisation loop in closed form (bitstream_coder.h), bits through a 64-bit accumulator as whole words.
#include "fpc_common.h"
#include "bitstream_coder.h"
#include <algorithm>

using namespace fpc_bs;

struct fpc_entropy_models {
    fpc::DevBuf cum;
    Tables T;
    int sizes[5];
    int words = 0;
    int device = 0;
};

namespace {

constexpr int WAVE = 64;
constexpr int MAX_FRAME = 2 + 16 + 32;                    // bits: two flags, a scalar index, two vector indices
constexpr int IMG = (31 + WAVE * MAX_FRAME) / 32 + 3;     // dwords of a step's image, with room for a 3-dword access
constexpr int MAX_L = 1 << 20;                            // keeps every bit count below 2^31
constexpr size_t LDS_LIMIT = 64 * 1024;                   // cumulative tables of one model set

// ---- fixed-length framing ----
__global__ __launch_bounds__(WAVE) void k_pack_fixed(Lay y, const int4* __restrict__ idx, int L, uint8_t* bytes,
                                                     long long stride, int* __restrict__ nbits) {
    __shared__ uint32_t img[IMG];
    const int lane = threadIdx.x, u = blockIdx.x;
    const Row row(bytes, u, stride);
    const int4* src = idx + (size_t)u * L;
    for (int i = lane; i < IMG; i += WAVE) img[i] = 0;
    __syncthreads();
    uint32_t off = 0;  // bits of the utterance so far
    bool invalid = false;
    for (int f0 = 0; f0 < L; f0 += WAVE) {
        uint64_t word = 0;
        int nb = 0;
        bool bad = false;
        if (f0 + lane < L) {
            const int4 q = src[f0 + lane];
            Frame f;
            bad = !frame_fields(y, q.x, q.y, q.z, q.w, f);
            word = (uint64_t)f.ind1 << 1 | (uint64_t)f.ind2;
            nb = 2;
            const int bs = f.ind1 ? y.b_sh : y.b_sl, ba = f.ind2 ? y.b_v0 : y.b_vl, bb = f.ind2 ? y.b_v1 : 0;
            word = (word << bs) | (uint32_t)f.scl;
            word = (word << ba) | (uint32_t)f.va;
            word = (word << bb) | (uint32_t)f.vb;
            nb += bs + ba + bb;
        }
        if (__any(bad)) {
            invalid = true;
            break;
        }
        int incl = nb;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const uint32_t total = (uint32_t)__shfl(incl, WAVE - 1);
        if (nb) {  // left-align the frame, shift it to its bit of the image: 96 bits over three dwords
            const uint32_t o = (off & 31u) + (uint32_t)(incl - nb);
            const int d = (int)(o >> 5), p = (int)(o & 31u);
            const uint64_t top = word << (64 - nb);
            const uint64_t hi = top >> p;
            const uint32_t lo = p ? (uint32_t)((top << (64 - p)) >> 32) : 0u;
            if (hi >> 32) atomicOr(&img[d], (uint32_t)(hi >> 32));
            if ((uint32_t)hi) atomicOr(&img[d + 1], (uint32_t)hi);
            if (lo) atomicOr(&img[d + 2], lo);
        }
        __syncthreads();
        const uint32_t d0 = off >> 5, nd = ((off + total) >> 5) - d0;  // dwords this step completed
        for (uint32_t i = lane; i < nd; i += WAVE) row.store(d0 + i, img[i]);
        const uint32_t carry = img[nd];
        __syncthreads();
        for (int i = lane; i < IMG; i += WAVE) img[i] = i ? 0u : carry;
        __syncthreads();
        off += total;
    }
    // the unfinished dword, then zeros to the end of the row; a refused utterance is zeros from the start
    uint32_t first_free = 0;
    if (!invalid) {
        first_free = (off + 31u) >> 5;
        if ((off & 31u) && lane == 0) row.store(off >> 5, img[0]);
    }
    __syncthreads();  // orders the stores above before the zeros of other lanes
    for (long long w = (long long)first_free + lane; w < row.words(); w += WAVE) row.store(w, 0u);
    if (lane == 0) nbits[u] = invalid ? -1 : (int)off;
}

__global__ __launch_bounds__(WAVE) void k_unpack_fixed(Lay y, const uint8_t* bytes, long long stride, int L,
                                                       int4* __restrict__ idx) {
    __shared__ uint32_t img[IMG];
    const int lane = threadIdx.x, u = blockIdx.x;
    const Row row(bytes, u, stride);
    int4* dst = idx + (size_t)u * L;
    const int len00 = y.frame_bits(false, false), len01 = y.frame_bits(false, true), len10 = y.frame_bits(true, false),
              len11 = y.frame_bits(true, true);
    const int stage = (31 + WAVE * std::max(std::max(len00, len01), std::max(len10, len11))) / 32 + 3;  // <= IMG
    uint32_t off = 0;
    for (int f0 = 0; f0 < L; f0 += WAVE) {
        const uint32_t d0 = off >> 5;
        for (int i = lane; i < stage; i += WAVE) img[i] = row.load((long long)d0 + i);
        __syncthreads();
        // phase 1: the chain over the flags, the same for every lane; lane t keeps where frame t starts
        const int nf = min(WAVE, L - f0);
        uint32_t pos = off & 31u, mine = 0;
        for (int t = 0; t < nf; ++t) {
            if (t == lane) mine = pos;
            const uint32_t d = pos >> 5, p = pos & 31u;
            const uint32_t fl = (uint32_t)((((uint64_t)img[d] << 32) | img[d + 1]) >> (62 - p)) & 3u;
            pos += fl == 3 ? len11 : fl == 2 ? len10 : fl == 1 ? len01 : len00;
        }
        // phase 2: 64 bits of the image from the frame's first bit, fields from the top
        if (lane < nf) {
            const uint32_t d = mine >> 5, p = mine & 31u;
            const uint64_t hi = ((uint64_t)img[d] << 32) | img[d + 1];
            uint64_t v = p ? (hi << p) | (img[d + 2] >> (32 - p)) : hi;
            auto take = [&v](int n) {
                const uint32_t r = n ? (uint32_t)(v >> (64 - n)) : 0u;
                v <<= n;
                return (int)r;
            };
            const bool ind1 = take(1), ind2 = take(1);
            int4 q = make_int4(-1, -1, -1, -1);
            if (ind1) q.x = take(y.b_sh);
            else if (y.n_lo) q.x = y.n_hi + take(y.b_sl);
            if (ind2) {
                q.y = take(y.b_v0);
                if (y.N1) q.z = take(y.b_v1);
            } else if (y.N_lo) {
                q.w = take(y.b_vl);
            }
            dst[f0 + lane] = q;
        }
        off += pos - (off & 31u);
        __syncthreads();
    }
}

// ---- entropy-coded framing ----
__device__ inline void load_tables(uint32_t* s_cum, const uint32_t* __restrict__ cum, int words) {
    for (int i = threadIdx.x; i < words; i += WAVE) s_cum[i] = cum[i];
    __syncthreads();
}

__global__ __launch_bounds__(WAVE) void k_pack_entropy(Lay y, Tables T, int words, const uint32_t* __restrict__ cum,
                                                       const int4* __restrict__ idx, int B, int L, uint8_t* bytes,
                                                       long long stride, int* __restrict__ nbits) {
    extern __shared__ uint32_t s_cum[];
    load_tables(s_cum, cum, words);
    const int u = blockIdx.x * WAVE + threadIdx.x;
    int first_free = 0;
    if (u < B) {
        BitWriter w(Row(bytes, u, stride));
        Encoder e;
        const int4* src = idx + (size_t)u * L;
        bool bad = false;
        int4 next = L ? src[0] : make_int4(0, 0, 0, 0);
        for (int i = 0; i < L; ++i) {
            const int4 q = next;
            if (i + 1 < L) next = src[i + 1];  // in flight while this frame is coded
            Frame f;
            if (!frame_fields(y, q.x, q.y, q.z, q.w, f)) {
                bad = true;
                break;
            }
            // lanes differ in which book a field uses, not in whether the coder runs: one call per field position
            e.put(w, s_cum, T, F1, f.ind1);
            e.put(w, s_cum, T, F2, f.ind2);
            if (f.has_scl) e.put(w, s_cum, T, f.ind1 ? SH : SL, f.scl);
            if (f.ind2 || f.has_vl) e.put(w, s_cum, T, f.ind2 ? V0 : VL, f.va);
            if (f.has_vb) e.put(w, s_cum, T, V1, f.vb);
        }
        if (!bad) {
            e.finish(w);
            nbits[u] = w.bits();
            first_free = w.finish();
        } else {
            nbits[u] = -1;
        }
    }
    __syncthreads();  // orders every lane's stores before the zeros other lanes write into its row
    // zeros from the first unused word to the end of each row (a refused utterance: the whole row), the workgroup together
    for (int t = 0; t < WAVE && blockIdx.x * WAVE + t < B; ++t) {
        const Row row(bytes, blockIdx.x * WAVE + t, stride);
        for (long long w = (long long)__shfl(first_free, t) + threadIdx.x; w < row.words(); w += WAVE) row.store(w, 0u);
    }
}

__global__ __launch_bounds__(WAVE) void k_unpack_entropy(Lay y, Tables T, int words, const uint32_t* __restrict__ cum,
                                                         const uint8_t* bytes, long long stride, int B, int L,
                                                         int4* __restrict__ idx) {
    extern __shared__ uint32_t s_cum[];
    load_tables(s_cum, cum, words);
    const int u = blockIdx.x * WAVE + threadIdx.x;
    if (u >= B) return;
    BitReader r(Row(bytes, u, stride));
    Decoder d;
    d.start(r);
    int4* dst = idx + (size_t)u * L;
    for (int i = 0; i < L; ++i) {
        const bool ind1 = d.get(r, s_cum, T, F1), ind2 = d.get(r, s_cum, T, F2);
        int4 q = make_int4(-1, -1, -1, -1);
        if (ind1 || y.n_lo) {  // one call per field position, whichever book a lane reads it from
            const int s = d.get(r, s_cum, T, ind1 ? SH : SL);
            q.x = ind1 ? s : y.n_hi + s;
        }
        if (ind2 || y.N_lo) {
            const int s = d.get(r, s_cum, T, ind2 ? V0 : VL);
            if (ind2) q.y = s;
            else q.w = s;
        }
        if (ind2 && y.N1) q.z = d.get(r, s_cum, T, V1);
        dst[i] = q;
    }
}

int make_layout(const int* sizes, Lay& y, const char* who) {
    FPC_REQUIRE(sizes, "%s: null sizes", who);
    FPC_REQUIRE(sizes[0] >= 1 && sizes[2] >= 1, "%s: the above-threshold books cannot be empty (n_hi=%d N_hi0=%d)", who,
                sizes[0], sizes[2]);
    for (int i = 0; i < 5; ++i)
        FPC_REQUIRE(sizes[i] >= 0 && sizes[i] <= MAX_SIZE, "%s: sizes[%d]=%d outside 0..%d", who, i, sizes[i], MAX_SIZE);
    y.n_hi = sizes[0], y.n_lo = sizes[1], y.N0 = sizes[2], y.N1 = sizes[3], y.N_lo = sizes[4];
    y.b_sh = width_of(y.n_hi), y.b_sl = width_of(y.n_lo), y.b_v0 = width_of(y.N0), y.b_v1 = width_of(y.N1),
    y.b_vl = width_of(y.N_lo);
    return FPC_OK;
}

int check_call(const char* who, const int* sizes, const fpc_entropy_models* m, const void* idx_dev, int B, int L,
               const void* bytes_dev, long long stride, Lay& y) {
    const int rc = make_layout(sizes, y, who);
    if (rc != FPC_OK) return rc;
    FPC_REQUIRE(B >= 0 && L >= 0 && L <= MAX_L && stride >= 0, "%s: bad shape B=%d L=%d stride=%lld", who, B, L, stride);
    FPC_REQUIRE((idx_dev || !B || !L) && ((uintptr_t)idx_dev & 15) == 0, "%s: idx_dev must be a 16-byte aligned device pointer",
                who);
    FPC_REQUIRE(bytes_dev || stride == 0, "%s: null bytes_dev with stride %lld", who, stride);
    if (!fpc::have_device()) {
        fpc::set_error("%s: no HIP device (libfpcodec has no CPU fallback)", who);
        return FPC_ERR_NO_DEVICE;
    }
    if (m) {
        FPC_REQUIRE(std::equal(sizes, sizes + 5, m->sizes), "%s: the models were created for other sizes", who);
        int dev = 0;
        FPC_HIP(hipGetDevice(&dev));
        FPC_REQUIRE(dev == m->device, "%s: the models live on device %d, current is %d", who, m->device, dev);
    }
    return FPC_OK;
}

}  // namespace

extern "C" int fpc_entropy_models_create(const int sizes[5], const uint32_t* cum_host, fpc_entropy_models** out) {
    FPC_REQUIRE(cum_host && out, "fpc_entropy_models_create: null argument");
    *out = nullptr;
    Lay y;
    const int rc = make_layout(sizes, y, "fpc_entropy_models_create");
    if (rc != FPC_OK) return rc;
    const int n[NTAB] = {2, 2, y.n_hi, y.n_lo, y.N0, y.N1, y.N_lo};
    Tables T;
    int words = 0;
    for (int t = 0; t < NTAB; ++t) {  // an absent book has no table: off stays in range, n = 0, never used
        T.off[t] = words, T.n[t] = n[t];
        if (!n[t]) continue;
        const uint32_t* c = cum_host + words;
        FPC_REQUIRE(c[0] == 0, "fpc_entropy_models_create: table %d starts at %u, not 0", t, c[0]);
        for (int i = 0; i < n[t]; ++i)
            FPC_REQUIRE(c[i + 1] > c[i], "fpc_entropy_models_create: table %d is not strictly increasing at %d", t, i);
        FPC_REQUIRE(c[n[t]] <= (uint32_t)MAX_SIZE, "fpc_entropy_models_create: table %d has total %u > %d", t, c[n[t]],
                    MAX_SIZE);
        words += n[t] + 1;
    }
    if ((size_t)words * sizeof(uint32_t) > LDS_LIMIT) {
        fpc::set_error("fpc_entropy_models_create: %d table entries do not fit %zu bytes of LDS", words, LDS_LIMIT);
        return FPC_ERR_CAPACITY;
    }
    if (!fpc::have_device()) {
        fpc::set_error("fpc_entropy_models_create: no HIP device (libfpcodec has no CPU fallback)");
        return FPC_ERR_NO_DEVICE;
    }
    auto* m = new fpc_entropy_models;
    m->T = T, m->words = words;
    std::copy(sizes, sizes + 5, m->sizes);
    hipError_t e = hipGetDevice(&m->device);
    if (e == hipSuccess) e = m->cum.upload(std::vector<uint32_t>(cum_host, cum_host + words));
    if (e != hipSuccess) {
        fpc::set_error("fpc_entropy_models_create: %s", hipGetErrorString(e));
        delete m;
        return FPC_ERR_HIP;
    }
    *out = m;
    return FPC_OK;
}

extern "C" void fpc_entropy_models_destroy(fpc_entropy_models* m) { delete m; }

// Fixed-length: the widest frame times L.  Entropy-coded: the coder's own worst case, derived, not measured --
//   every pass of the renormalisation loop doubles the range R = high - low + 1 and ends up as exactly one bit of output
//   (an agree-step emits its bit, an underflow-step a pending one), and the end adds 2 bits: nbits = passes + 2;
//   a field narrows R to floor(R c1 / T) - floor(R c0 / T) >= R (c1 - c0) / T - 1, with a count c1 - c0 >= 1, a total
//   T <= 2^16 and R > 2^30 whenever a field is coded (the loop only stops there; R = 2^32 at the start): a factor
//   >= 2^-16 - 2^-30 = 2^-16 (1 - 2^-14), i.e. at most 16 + 2^-13 doublings to make up for;
//   R starts at 2^32 and never exceeds it, so passes <= F (16 + 2^-13) over the F fields of an utterance.
// F counts the fields of the fullest frame: two flags, a scalar, and the larger of the two vector alternatives.
extern "C" long long fpc_bitstream_bound(const int sizes[5], int entropy, int L) {
    Lay y;
    const int rc = make_layout(sizes, y, "fpc_bitstream_bound");
    if (rc != FPC_OK) return rc;
    FPC_REQUIRE(L >= 0 && L <= MAX_L, "fpc_bitstream_bound: L=%d outside 0..%d", L, MAX_L);
    long long bits;
    if (entropy) {
        const long long F = (long long)L * (3 + std::max(1 + (y.N1 ? 1 : 0), y.N_lo ? 1 : 0));
        bits = 16 * F + (F >> 13) + 2;
    } else {
        bits = (long long)L * std::max(std::max(y.frame_bits(false, false), y.frame_bits(false, true)),
                                       std::max(y.frame_bits(true, false), y.frame_bits(true, true)));
    }
    return (bits + 7) / 8;
}

extern "C" int fpc_bitstream_pack(const int sizes[5], const fpc_entropy_models* m, const int32_t* idx_dev, int B, int L,
                                  uint8_t* bytes_dev, long long stride, int32_t* nbits_dev, fpc_stream s) {
    Lay y;
    const int rc = check_call("fpc_bitstream_pack", sizes, m, idx_dev, B, L, bytes_dev, stride, y);
    if (rc != FPC_OK) return rc;
    FPC_REQUIRE(nbits_dev, "fpc_bitstream_pack: null nbits_dev");
    if (B == 0) return FPC_OK;
    const int4* idx = reinterpret_cast<const int4*>(idx_dev);
    if (m)
        hipLaunchKernelGGL(k_pack_entropy, dim3((B + WAVE - 1) / WAVE), dim3(WAVE), m->words * sizeof(uint32_t),
                           static_cast<hipStream_t>(s), y, m->T, m->words, m->cum.as<uint32_t>(), idx, B, L, bytes_dev,
                           stride, nbits_dev);
    else
        hipLaunchKernelGGL(k_pack_fixed, dim3(B), dim3(WAVE), 0, static_cast<hipStream_t>(s), y, idx, L, bytes_dev, stride,
                           nbits_dev);
    FPC_HIP(hipGetLastError());
    return FPC_OK;
}

extern "C" int fpc_bitstream_unpack(const int sizes[5], const fpc_entropy_models* m, const uint8_t* bytes_dev,
                                    long long stride, int B, int L, int32_t* idx_dev, fpc_stream s) {
    Lay y;
    const int rc = check_call("fpc_bitstream_unpack", sizes, m, idx_dev, B, L, bytes_dev, stride, y);
    if (rc != FPC_OK) return rc;
    if (B == 0 || L == 0) return FPC_OK;
    int4* idx = reinterpret_cast<int4*>(idx_dev);
    if (m)
        hipLaunchKernelGGL(k_unpack_entropy, dim3((B + WAVE - 1) / WAVE), dim3(WAVE), m->words * sizeof(uint32_t),
                           static_cast<hipStream_t>(s), y, m->T, m->words, m->cum.as<uint32_t>(), bytes_dev, stride, B, L,
                           idx);
    else
        hipLaunchKernelGGL(k_unpack_fixed, dim3(B), dim3(WAVE), 0, static_cast<hipStream_t>(s), y, bytes_dev, stride, L,
                           idx);
    FPC_HIP(hipGetLastError());
    return FPC_OK;
}
