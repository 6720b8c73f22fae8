// FLAC files, device half: the subframes of every frame of a batch -> float32 interleaved samples, which K0 (ww_decode.hip) then
// reads as a WW_FMT_F32 file (RFC 9639 sections 9.2-9.3: CONSTANT, VERBATIM, FIXED 0-4, LPC 1-32, wasted bits, Rice / Rice2 / escape
// partitions, left/side, side/right, mid/side).
//
// The host (ww_flac_index.h) has verified every header's CRC-8 and every frame's CRC-16 and built the frame index; it uploads the frames'
// bytes and the index with the staging.  One lane decodes one frame: the subframes of a frame are sequential in the bitstream (channel
// 2 starts where channel 1's residual ends), and the prediction is a serial recurrence per subframe, so a frame is the natural unit of
// independent work.  The last 32 samples of the subframe being restored and its predictor coefficients sit in LDS, one column per lane.
// Prediction is exact 64-bit integer arithmetic.  Every read is bounded by the frame's byte range; a bitstream that is inconsistent
// (reserved codes, a negative LPC shift, a partition layout the block does not allow, a sample outside its bit width, reading past the
// frame) zeroes its file's row: the descriptor's n_frames becomes 0 -- what K0 writes for an unreadable file -- and the file is counted
// once in g_flac_errors (ww_flac_errors()).  Floats are x * 2^-(bps-1), soundfile's scaling for a WAV of the same integers.
#include "ww_internal.h"

namespace ww {

__device__ unsigned int g_flac_errors;

namespace {

constexpr int kFlacThreads = 64;
constexpr int kHist = 32;              // ring of the last 32 samples = the largest LPC order

// MSB-first bit reader over [p, p + n_bytes): a 64-bit window, refilled a byte at a time; bytes past the end read as zero and are
// counted, so that a run past the frame is detected (over()) instead of read.
struct Bits {
    const uint8_t* p;
    int64_t n_bytes, next;             // next byte to load
    uint64_t buf;                      // the top `have` bits are valid
    int have;
    __host__ __device__ void refill() {
        while (have <= 56) {
            const uint64_t b = next < n_bytes ? uint64_t(p[next]) : 0;
            ++next;
            buf |= b << (56 - have);
            have += 8;
        }
    }
    __host__ __device__ bool over() const { return next * 8 - have > n_bytes * 8; }   // more bits consumed than the frame holds
    __host__ __device__ uint32_t get(int n) {   // n <= 32
        if (n == 0) return 0;
        if (have < n) refill();
        const uint32_t v = uint32_t(buf >> (64 - n));
        buf <<= n;
        have -= n;
        return v;
    }
    __host__ __device__ int32_t sget(int n) {   // two's complement of n <= 32 bits
        if (n == 0) return 0;
        const uint32_t v = get(n);
        return n == 32 ? int32_t(v) : int32_t(v << (32 - n)) >> (32 - n);
    }
    // zeros before the next 1 (the 1 consumed); -1 once the run exceeds `limit` or leaves the frame
    __host__ __device__ int64_t unary(int64_t limit) {
        int64_t q = 0;
        for (;;) {
            if (have == 0 || buf == 0) {
                q += have;
                buf = 0;
                have = 0;
                if (q > limit || next > n_bytes) return -1;
                refill();
                continue;
            }
            const int z = __builtin_clzll(buf);
            q += z;
            buf = z == 63 ? 0 : buf << (z + 1);
            have -= z + 1;
            return q > limit ? -1 : q;
        }
    }
};

struct Lds {
    int32_t* hist;                     // [kHist][kFlacThreads]: this lane's column
    int32_t* coef;                     // [kHist][kFlacThreads]
    __host__ __device__ int32_t& h(int64_t t) const { return hist[(t & (kHist - 1)) * kFlacThreads]; }
    __host__ __device__ int32_t& c(int j) const { return coef[j * kFlacThreads]; }
};

// One subframe into out[t * stride] (int32, wasted bits restored).  sbps = the subframe's sample width (the side channel's is bps + 1).
// false = inconsistent bitstream.
__host__ __device__ bool subframe(Bits& br, int bs, int sbps, int32_t* out, int stride, const Lds& L) {
    if (br.get(1)) return false;                                  // zero pad bit
    const int type = int(br.get(6));
    int wasted = 0;
    if (br.get(1)) {
        const int64_t k = br.unary(32);
        if (k < 0) return false;
        wasted = int(k) + 1;
    }
    if (wasted >= sbps) return false;
    sbps -= wasted;
    const int64_t lo = -(int64_t(1) << (sbps - 1)), hi = (int64_t(1) << (sbps - 1)) - 1;
    if (type == 0) {                                              // CONSTANT
        const int32_t v = br.sget(sbps) * (1 << wasted);
        for (int t = 0; t < bs; ++t) out[int64_t(t) * stride] = v;
        return !br.over();
    }
    if (type == 1) {                                              // VERBATIM
        for (int t = 0; t < bs; ++t) out[int64_t(t) * stride] = br.sget(sbps) * (1 << wasted);
        return !br.over();
    }
    int order, shift = 0;
    bool lpc;
    if (type >= 8 && type <= 12) { lpc = false; order = type - 8; }
    else if (type >= 32) { lpc = true; order = type - 31; }
    else return false;                                            // reserved
    if (order > bs) return false;
    for (int t = 0; t < order; ++t) {                             // warm-up samples
        const int32_t v = br.sget(sbps);
        L.h(t) = v;
        out[int64_t(t) * stride] = v * (1 << wasted);
    }
    if (lpc) {
        const int prec = int(br.get(4)) + 1;
        if (prec == 16) return false;
        shift = br.sget(5);
        if (shift < 0) return false;
        for (int j = 0; j < order; ++j) L.c(j) = br.sget(prec);
    }
    // residual
    const int method = int(br.get(2));
    if (method > 1) return false;
    const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
    const int porder = int(br.get(4));
    const int parts = 1 << porder;
    if (porder > 0 && ((bs & (parts - 1)) || (bs >> porder) < order)) return false;
    if (porder == 0 && bs < order) return false;
    if (br.over()) return false;
    int t = order;
    for (int part = 0; part < parts; ++part) {
        const int end = (part + 1) * (bs >> porder);
        const int k = int(br.get(pbits));
        const int raw = k == esc ? int(br.get(5)) : -1;
        const int64_t qlim = k == esc ? 0 : (int64_t(1) << (32 - k)) - 1;
        for (; t < end; ++t) {
            int64_t r;
            if (raw >= 0) r = br.sget(raw);
            else {
                const int64_t q = br.unary(qlim);
                if (q < 0) return false;
                const uint64_t u = (uint64_t(q) << k) | br.get(k);
                r = int64_t(u >> 1) ^ -int64_t(u & 1);
            }
            int64_t pred;
            if (!lpc) {
                switch (order) {
                    case 0: pred = 0; break;
                    case 1: pred = L.h(t - 1); break;
                    case 2: pred = 2 * int64_t(L.h(t - 1)) - L.h(t - 2); break;
                    case 3: pred = 3 * int64_t(L.h(t - 1)) - 3 * int64_t(L.h(t - 2)) + L.h(t - 3); break;
                    default: pred = 4 * int64_t(L.h(t - 1)) - 6 * int64_t(L.h(t - 2)) + 4 * int64_t(L.h(t - 3)) - L.h(t - 4); break;
                }
            } else {
                int64_t s = 0;
                for (int j = 0; j < order; ++j) s += int64_t(L.c(j)) * L.h(t - 1 - j);
                pred = s >> shift;
            }
            const int64_t v = pred + r;
            if (v < lo || v > hi) return false;
            L.h(t) = int32_t(v);
            out[int64_t(t) * stride] = int32_t(v) * (1 << wasted);
        }
        if (br.over()) return false;
    }
    return !br.over();
}

// One frame (bytes from its header on) -> float32 at out_i32 + sample_off * nch (through int32 in place).  false = inconsistent.
__host__ __device__ bool decode_frame(const uint8_t* comp, const FlacFrame& f, int nch, int bps, int32_t* out_i32, const Lds& L) {
    const int bs = f.block_size, ca = f.chan_assign;
    int32_t* out = out_i32 + f.sample_off * nch;
    Bits br{comp + f.byte_off + f.header_len, int64_t(f.byte_len) - f.header_len - 2, 0, 0, 0};
    for (int ch = 0; ch < nch; ++ch) {
        const bool side = (ca == 8 && ch == 1) || (ca == 9 && ch == 0) || (ca == 10 && ch == 1);
        if (!subframe(br, bs, bps + (side ? 1 : 0), out + ch, nch, L)) return false;
    }
    // channel decorrelation and the float scaling, in place
    const float scale = ldexpf(1.0f, -(bps - 1));
    float* outf = reinterpret_cast<float*>(out);
    for (int t = 0; t < bs; ++t) {
        int32_t* s = out + int64_t(t) * nch;
        if (ca >= 8) {
            int32_t a = s[0], b = s[1];
            if (ca == 8) b = a - b;                                 // left, side -> left, right
            else if (ca == 9) a = a + b;                           // side, right -> left, right
            else {                                                  // mid, side -> left, right
                const int32_t m = int32_t(uint32_t(a) << 1) | (b & 1);
                a = (m + b) >> 1;
                b = (m - b) >> 1;
            }
            outf[int64_t(t) * nch] = float(a) * scale;
            outf[int64_t(t) * nch + 1] = float(b) * scale;
        } else {
            for (int ch = 0; ch < nch; ++ch) outf[int64_t(t) * nch + ch] = float(s[ch]) * scale;
        }
    }
    return true;
}

__global__ __launch_bounds__(kFlacThreads) void flac_decode_kernel(uint8_t* __restrict__ raw, FlacClip* __restrict__ clips, int n_clips,
                                                                   int64_t n_frames, ww_clip_desc* __restrict__ descs) {
    __shared__ int32_t hist[kHist * kFlacThreads], coef[kHist * kFlacThreads];
    const int64_t g = int64_t(blockIdx.x) * kFlacThreads + threadIdx.x;
    if (g >= n_frames) return;
    int lo = 0, hi = n_clips - 1;                                  // the clip whose frames hold g: last first_frame <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (clips[mid].first_frame <= g) lo = mid; else hi = mid - 1;
    }
    FlacClip& c = clips[lo];
    const FlacFrame f = reinterpret_cast<const FlacFrame*>(raw + c.frames_off)[g - c.first_frame];
    if (!decode_frame(raw + c.comp_off, f, c.channels, c.bps, reinterpret_cast<int32_t*>(raw + c.dec_off), Lds{hist + threadIdx.x, coef + threadIdx.x})) {
        if (atomicExch(&c.err, 1) == 0) {
            atomicAdd(&g_flac_errors, 1u);
            descs[c.clip].n_frames = 0;
        }
    }
}

}  // namespace

__attribute__((visibility("default"))) int launch_flac_decode(uint8_t* raw_dev, FlacClip* clips_dev, int n_flac, int64_t n_frames_total,
                                                                ww_clip_desc* descs_dev, hipStream_t stream) {
    if (n_flac <= 0 || n_frames_total <= 0) return WW_OK;
    const int64_t blocks = (n_frames_total + kFlacThreads - 1) / kFlacThreads;
    return launch<flac_decode_kernel>(dim3(unsigned(blocks)), dim3(kFlacThreads), 0, stream, raw_dev, clips_dev, n_flac, n_frames_total, descs_dev);
}

int flac_errors(unsigned int* count) {
    WW_HIP(hipMemcpyFromSymbol(count, HIP_SYMBOL(g_flac_errors), sizeof(unsigned int)));
    return WW_OK;
}

}  // namespace ww
