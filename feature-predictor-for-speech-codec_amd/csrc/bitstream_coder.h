// bitstream_coder.h -- the per-stream pieces of csrc/bitstream.hip: frame layout, row access in MSB-first 32-bit words, and
// the static arithmetic coder of fpcodec_amd/bitstream.py (Witten-Neal-Cleary, 32-bit range) with its renormalisation loop
// in closed form.  Everything here is integer work of ONE stream (one lane); it compiles for the host too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fpc_bs {

constexpr uint32_t HALF = 0x80000000u, QTR = 0x40000000u;
constexpr int MAX_SIZE = 1 << 16;  // entries of one codebook (= _MAXTOT of bitstream.py: every symbol keeps a count >= 1)
// tables of a model set in stream order of their first use: f1 f2 scl_hi scl_lo v0 v1 vlo
enum { F1, F2, SH, SL, V0, V1, VL, NTAB };

inline int width_of(int n) {  // _bits of bitstream.py
    int b = 0;
    while ((1 << b) < n) ++b;
    return b;
}

// sizes = (n_hi, n_lo, N_hi0, N_hi1, N_lo) and the fixed-length field widths of bitstream.Layout
struct Lay {
    int n_hi, n_lo, N0, N1, N_lo;
    int b_sh, b_sl, b_v0, b_v1, b_vl;
    __host__ __device__ int frame_bits(bool ind1, bool ind2) const {
        return 2 + (ind1 ? b_sh : b_sl) + (ind2 ? b_v0 + b_v1 : b_vl);  // widths of absent books are 0
    }
};

// One frame's symbols {scalar, vq stage 1, vq stage 2, below-threshold vq} as the encoder writes them -> the fields of the
// frame.  false: the symbols contradict the layout (what bitstream.pack asserts on): an index past its table, a
// below-threshold symbol missing where a book exists, a symbol present where none is possible.
struct Frame {
    bool ind1, ind2;
    int scl, va, vb;  // scalar field (hi or lo book, offset removed), v0 | vlo, v1
    bool has_scl, has_vb, has_vl;
};
__host__ __device__ inline bool frame_fields(const Lay& y, int s, int v0, int v1, int vl, Frame& f) {
    f.ind1 = s >= 0 && s < y.n_hi;
    f.ind2 = v0 >= 0;
    f.scl = f.va = f.vb = 0;
    f.has_scl = f.has_vb = f.has_vl = false;
    if (f.ind1) {
        f.scl = s, f.has_scl = true;
    } else if (y.n_lo) {
        if (s < y.n_hi || s - y.n_hi >= y.n_lo) return false;
        f.scl = s - y.n_hi, f.has_scl = true;
    } else if (s >= 0) {
        return false;
    }
    if (f.ind2) {
        if (v0 >= y.N0) return false;
        f.va = v0;
        if (y.N1) {
            if (v1 < 0 || v1 >= y.N1) return false;
            f.vb = v1, f.has_vb = true;
        }
    } else if (y.N_lo) {
        if (vl < 0 || vl >= y.N_lo) return false;
        f.va = vl, f.has_vl = true;
    } else if (vl >= 0) {
        return false;
    }
    return true;
}

// A row of the byte buffer seen as 32-bit words whose MSB is the earlier bit.  Bytes at or beyond `stride` do not exist:
// never written, read as 0.  A word that lies whole inside a 4-aligned row moves as one dword, anything else byte by byte.
struct Row {
    uint8_t* p;
    long long stride;
    bool aligned;
    __host__ __device__ Row(const uint8_t* base, long long row, long long stride_)
        : p(const_cast<uint8_t*>(base) + row * stride_), stride(stride_), aligned(((uintptr_t)p & 3) == 0) {}
    __host__ __device__ void store(long long w, uint32_t v) const {
        const long long o = 4 * w;
        if (aligned && o + 4 <= stride) {
            *reinterpret_cast<uint32_t*>(p + o) = __builtin_bswap32(v);
        } else {
            for (int k = 0; k < 4; ++k)
                if (o + k < stride) p[o + k] = (uint8_t)(v >> (24 - 8 * k));
        }
    }
    __host__ __device__ uint32_t load(long long w) const {
        const long long o = 4 * w;
        if (aligned && o + 4 <= stride) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(p + o));
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k)
            if (o + k < stride) v |= (uint32_t)p[o + k] << (24 - 8 * k);
        return v;
    }
    __host__ __device__ long long words() const { return (stride + 3) >> 2; }
};

// 64-bit accumulator flushed as whole words; keeps counting past the end of the row (Row::store drops what does not fit)
struct BitWriter {
    Row row;
    uint64_t acc = 0;
    int nacc = 0;  // < 32 between calls
    int wpos = 0;
    __host__ __device__ explicit BitWriter(const Row& r) : row(r) {}
    __host__ __device__ void put(uint32_t v, int n) {  // n <= 32, v < 2^n
        acc = (acc << n) | v;
        nacc += n;
        if (nacc >= 32) {
            nacc -= 32;
            row.store(wpos++, (uint32_t)(acc >> nacc));
        }
    }
    __host__ __device__ void run(uint32_t bit, uint32_t r) {  // r copies of one bit, word-wise
        const uint32_t fill = bit ? 0xffffffffu : 0u;
        for (; r >= 32; r -= 32) put(fill, 32);
        put(r ? fill >> (32 - r) : 0u, (int)r);
    }
    __host__ __device__ int bits() const { return 32 * wpos + nacc; }
    // writes the last partial word (zero filled); returns the first word of the row that holds no bit
    __host__ __device__ int finish() {
        if (!nacc) return wpos;
        row.store(wpos, (uint32_t)(acc << (32 - nacc)));
        return wpos + 1;
    }
};

// the next word of the row is always loaded one refill ahead, so its latency runs beside the coder's arithmetic
struct BitReader {
    Row row;
    uint64_t buf = 0;
    int nbuf = 0;
    long long wpos = 1;
    uint32_t ahead;
    __host__ __device__ explicit BitReader(const Row& r) : row(r), ahead(r.load(0)) {}
    __host__ __device__ uint32_t get(int n) {  // n <= 32
        if (nbuf < n) {
            buf = (buf << 32) | ahead;
            ahead = row.load(wpos++);
            nbuf += 32;
        }
        nbuf -= n;
        const uint32_t v = (uint32_t)(buf >> nbuf);
        return n >= 32 ? v : v & ((1u << n) - 1u);
    }
};

// floor(rng * c / tot) of the reference, rng <= 2^32, c <= tot <= 2^16: long division in base 2^16, two 32-bit divisions.
// c == tot gives rng itself; otherwise c <= 65535 and x = rng * c < 2^48, so a = x >> 16 fits 32 bits, a % tot < 2^16,
// and the second dividend (a % tot) << 16 | (x & 0xffff) fits 32 bits too.
__host__ __device__ inline uint64_t scale(uint64_t rng, uint32_t c, uint32_t tot) {
    if (c == tot) return rng;
    const uint64_t x = rng * c;
    const uint32_t a = (uint32_t)(x >> 16), b = (uint32_t)x & 0xffffu;
    const uint32_t q1 = a / tot, r1 = a - q1 * tot;
    return ((uint64_t)q1 << 16) + ((r1 << 16) | b) / tot;
}

// The renormalisation loop of entropy_pack / entropy_unpack in closed form.  After a symbol narrowed [low, high]:
//   k = clz(low ^ high) leading bits agree.  The loop's first two branches shift them out one by one; nothing else can
//       happen before they are gone (the third branch needs low < HALF <= high).  Then low = 0..., high = 1....
//   j = the run of positions below the top bit where low has 1 and high has 0.  Each is one pass through the third branch
//       (low >= QTR and high < HALF + QTR), which deletes bit 30 of both and keeps bit 31; after it low < HALF <= high
//       still holds, so no agree-step can follow, and the loop ends when the run does.
// One pass of the third branch is x -> 2 x - 2^31 (+ 1 for high, + the next input bit for the decoder's val), so j passes
// are x -> 2^j x - 2^31 (2^j - 1) + fill, which modulo 2^32 is ((x << j) ^ HALF) | fill for j >= 1; the true value lies
// in [0, 2^32), so the 32-bit result is it.  The agree-steps are plain shifts (subtracting HALF clears the bit shifted out).
struct Renorm {
    int k, j;
    uint32_t agreed;  // the k bits shifted out, first one at bit k - 1
};
__host__ __device__ inline Renorm renorm(uint32_t& low, uint32_t& high) {
    Renorm r;
    const uint32_t x = low ^ high;
    r.k = x ? __builtin_clz(x) : 32;  // low < high always (a count >= 1 leaves >= 2^14 values): 32 cannot happen
    r.agreed = r.k ? low >> (32 - r.k) : 0u;
    if (r.k) {
        low = r.k < 32 ? low << r.k : 0u;
        high = r.k < 32 ? (high << r.k) | ((1u << r.k) - 1u) : 0xffffffffu;
    }
    const uint32_t m = (low & ~high) << 1;  // bit 0 is 0, so ~m != 0
    r.j = __builtin_clz(~m);                // <= 31
    if (r.j) {
        low = (low << r.j) ^ HALF;
        high = ((high << r.j) ^ HALF) | ((1u << r.j) - 1u);
    }
    return r;
}

// cumulative tables of all fields in one array (LDS in the kernels): table t has n[t] + 1 entries from off[t]
struct Tables {
    int off[NTAB], n[NTAB];
};

struct Encoder {
    uint32_t low = 0, high = 0xffffffffu, pend = 0;
    __host__ __device__ void put(BitWriter& w, const uint32_t* cum, const Tables& T, int t, int sym) {
        const uint32_t* c = cum + T.off[t];
        const uint32_t tot = c[T.n[t]];
        const uint64_t rng = (uint64_t)high - low + 1;
        high = (uint32_t)(low + scale(rng, c[sym + 1], tot) - 1);
        low = (uint32_t)(low + scale(rng, c[sym], tot));
        const Renorm r = renorm(low, high);
        if (r.k) {  // emit(first bit): the bit, the pending run inverted; the other k - 1 agreed bits follow as they are
            const uint32_t b0 = (r.agreed >> (r.k - 1)) & 1u;
            w.put(b0, 1);
            w.run(b0 ^ 1u, pend);
            w.put(r.agreed & ((1u << (r.k - 1)) - 1u), r.k - 1);
            pend = 0;
        }
        pend += (uint32_t)r.j;
    }
    __host__ __device__ void finish(BitWriter& w) {
        const uint32_t b = low < QTR ? 0u : 1u;
        w.put(b, 1);
        w.run(b ^ 1u, pend + 1);
    }
};

struct Decoder {
    uint32_t low = 0, high = 0xffffffffu, val = 0;
    __host__ __device__ void start(BitReader& r) { val = r.get(32); }
    __host__ __device__ int get(BitReader& rd, const uint32_t* cum, const Tables& T, int t) {
        const uint32_t* c = cum + T.off[t];
        const int n = T.n[t];
        const uint32_t tot = c[n];
        const uint64_t rng = (uint64_t)high - low + 1;  // 2^30 < rng <= 2^32
        // target = ((val - low + 1) * tot - 1) // rng, < tot <= 2^16.  num < 2^48 and rng are exact in float64 and the
        // quotient of a correctly rounded division is off by < 2^-36, so its truncation is the floor or one beside it:
        // the two comparisons settle which
        const uint64_t num = ((uint64_t)(val - low) + 1) * tot - 1;
        uint64_t q = (uint64_t)((double)num / (double)rng);
        if (q * rng > num) --q;
        else if ((q + 1) * rng <= num) ++q;
        const uint32_t target = (uint32_t)q;
        int lo = 0, hi = n;  // largest lo with c[lo] <= target (searchsorted side = right, minus 1); c[0] = 0
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (c[mid] <= target) lo = mid;
            else hi = mid;
        }
        high = (uint32_t)(low + scale(rng, c[lo + 1], tot) - 1);
        low = (uint32_t)(low + scale(rng, c[lo], tot));
        const Renorm r = renorm(low, high);  // val follows low: the same shifts, fresh bits shifted in
        if (r.k) val = (r.k < 32 ? val << r.k : 0u) | rd.get(r.k);
        if (r.j) val = ((val << r.j) ^ HALF) | rd.get(r.j);
        return lo;
    }
};

}  // namespace fpc_bs
