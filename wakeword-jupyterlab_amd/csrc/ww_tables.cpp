// Host-side construction of the front-end tables and of the packed weight image.  Pure CPU code
// (double precision, rounded once to float32): callable without a GPU through the C ABI so the
// CPU test-suite can check it against the oracle.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ww_internal.h"

namespace ww {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
const char* last_error() { return g_err; }

// ---- Slaney mel scale: librosa.hz_to_mel / mel_to_hz with htk=False ---------------------------
static double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
    const double logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
    const double logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// librosa.filters.mel(sr=16000, n_fft=2048, n_mels=80, fmin=0, fmax=8000, norm='slaney', dtype=float32):
// triangle stored as float32, then scaled by the float64 area normaliser and rounded again.
void build_mel_filterbank(float* out) {
    const int n_edges = kMels + 2;
    std::vector<double> edges(n_edges);
    const double m0 = hz_to_mel(0.0), m1 = hz_to_mel(8000.0);
    const double step = (m1 - m0) / (n_edges - 1);          // np.linspace: start + i*step, last = stop
    for (int i = 0; i < n_edges; ++i) edges[i] = mel_to_hz(i == n_edges - 1 ? m1 : m0 + i * step);
    for (int i = 0; i < kMels; ++i) {
        const double fd0 = edges[i + 1] - edges[i], fd1 = edges[i + 2] - edges[i + 1];
        const double enorm = 2.0 / (edges[i + 2] - edges[i]);
        for (int k = 0; k < kBins; ++k) {
            const double f = k * (double(WW_SAMPLE_RATE) / kNfft);
            const double lower = -(edges[i] - f) / fd0, upper = (edges[i + 2] - f) / fd1;
            const double tri = std::fmax(0.0, std::fmin(lower, upper));
            out[i * kBins + k] = float(double(float(tri)) * enorm);
        }
    }
}

void build_hann(double* w) {
    for (int n = 0; n < kNfft; ++n) w[n] = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / kNfft);
}

// Modified Bessel function I0 by its power series (x <= 15: 40 terms reach double precision).
static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 200; ++k) {
        term *= q / (double(k) * double(k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// resampy.filters.sinc_window(num_zeros=64, precision=9, window=kaiser(beta), rolloff): the right half of
// kaiser(2n+1, beta) * rolloff * sinc(rolloff * x), x = linspace(0, 64, n + 1), n = 64 * 512.
void build_kaiser_best(float* out) {
    const int n = 64 * 512;
    const double beta = 14.769656459379492, rolloff = 0.9475937167399596;
    const double i0b = bessel_i0(beta);
    for (int i = 0; i <= n; ++i) {
        const double x = 64.0 * double(i) / double(n);
        const double a = M_PI * rolloff * x;
        const double sinc = i == 0 ? 1.0 : std::sin(a) / a;
        const double r = double(i) / double(n);
        const double taper = bessel_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / i0b;
        out[i] = float(taper * rolloff * sinc);
    }
}

static double2 twiddle_d(int N, long e) {   // W_N^e = exp(-2*pi*i*e/N), argument reduced exactly
    e %= N;
    const double a = -2.0 * M_PI * double(e) / double(N);
    double2 r;
    r.x = std::cos(a);
    r.y = std::sin(a);
    return r;
}
static float2 twiddle(int N, long e) {
    const double2 t = twiddle_d(N, e);
    return make_float2(float(t.x), float(t.y));
}

int build_logmel_tables(LogmelTables* t) {
    std::memset(t, 0, sizeof(*t));
    std::vector<double> w(kNfft);
    build_hann(w.data());
    for (int n = 0; n < kNfft; ++n) { t->window[n] = float(w[n]); t->window_d[n] = w[n]; }
    for (int k1 = 1; k1 < 8; ++k1)
        for (int n = 0; n < 128; ++n) { t->tw1[k1 - 1][n] = twiddle(1024, long(n) * k1); t->tw1_d[k1 - 1][n] = twiddle_d(1024, long(n) * k1); }
    for (int k2 = 1; k2 < 8; ++k2)
        for (int n = 0; n < 16; ++n) { t->tw2[k2 - 1][n] = twiddle(128, long(n) * k2); t->tw2_d[k2 - 1][n] = twiddle_d(128, long(n) * k2); }
    for (int k = 0; k < 512; ++k) { t->twp[k] = twiddle(2048, k == 0 ? 512 : k); t->twp_d[k] = twiddle_d(2048, k == 0 ? 512 : k); }
    for (int k = 0; k < 1024; ++k) t->twr[k] = twiddle(2048, k);
    build_kaiser_best(t->kaiser_best);

    std::vector<float> M(size_t(kMels) * kBins);
    build_mel_filterbank(M.data());
    for (int f = 0; f < kMels; ++f) {
        float wmax = 0.f;
        for (int k = 0; k < kBins; ++k) wmax = std::fmax(wmax, M[f * kBins + k]);
        t->band_wmax[f] = wmax;
        t->band_bins[f] = 1.0f / wmax;              // the kernel's multiplier: P_b / wmax_b
    }
    struct Piece { int m, f, pos; };
    std::vector<Piece> pieces;
    int pos = 0;
    for (int f = 0; f < kMels; ++f) {
        int lo = -1, hi = -1;
        for (int k = 0; k < kBins; ++k)
            if (M[f * kBins + k] != 0.0f) { if (lo < 0) lo = k; hi = k; }
        if (lo < 1 || hi > 1023) return fail(WW_EINVAL, "mel filter %d touches bin 0 or 1024", f);
        for (int k = lo; k <= hi; ++k)   // support must be one contiguous run
            if (M[f * kBins + k] == 0.0f) return fail(WW_EINVAL, "mel filter %d has a hole at bin %d", f, k);
        t->filt_p0[f] = pos;
        for (int m = lo / kPieceLen; m <= hi / kPieceLen; ++m) pieces.push_back({m, f, pos++});
        t->filt_cnt[f] = pos - t->filt_p0[f];
    }
    const int real = int(pieces.size());
    if (real > kPieces) return fail(WW_EINVAL, "%d mel pieces exceed the %d slots", real, kPieces);
    std::stable_sort(pieces.begin(), pieces.end(), [](const Piece& a, const Piece& b) { return a.m < b.m; });
    // padding pieces (all-zero weights) reuse the last window and write to spare output positions
    while (int(pieces.size()) < kPieces) pieces.push_back({pieces.back().m, -1, pos++});
    // lanes of the four ds_read_b128 hardware groups of a wave64 (MI355X_MICROARCH.md, LDS table)
    static const int group_lanes[4][16] = {
        {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
        {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
        {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
        {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    for (int i = 0; i < kPieces; ++i) {
        const int c = i / 64, g = (i % 64) / 16, j = i % 16;
        const int slot = c * 64 + group_lanes[g][j];
        const Piece& pc = pieces[i];
        t->piece_info[slot] = (pc.m * kPieceLen) | (pc.pos << 16);
        for (int b = 0; b < kPieceLen; ++b) {
            const float w = pc.f >= 0 ? M[pc.f * kBins + pc.m * kPieceLen + b] : 0.0f;
            t->piece_w[b / 4][slot][b % 4] = w;
        }
    }
    return real;
}

// ---- packed weights --------------------------------------------------------------------------
PackedLayout packed_layout(int n_conv) {
    PackedLayout L{};
    L.n_conv = n_conv;
    L.c_last = n_conv == 3 ? 128 : 64;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t at = o; o += (n + 3) & ~int64_t(3); return at; };   // 16-byte aligned blocks
    L.conv1_w = take(32 * 9);
    L.conv1_b = take(32);
    L.conv2_w = take(2 * 144 * 64);
    L.conv2_b = take(64);
    L.conv3_w = n_conv == 3 ? take(4 * 288 * 64) : -1;
    L.conv3_b = n_conv == 3 ? take(128) : -1;
    L.l0_w = take(int64_t(L.c_last) * kGateCols);
    L.l0_b = take(kGateCols);
    L.l1_w = take(int64_t(kHidden) * kGateCols);
    L.l1_b = take(kGateCols);
    L.fc_w = take(2 * kHidden);
    L.fc_b = take(4);
    L.conv2_hs = take(64);
    L.conv3_h = n_conv == 3 ? take(8 * 18 * 2 * 64 * 4) : -1;
    L.conv3_hs = n_conv == 3 ? take(128) : -1;
    L.conv1_h = take(2 * 64 * 4);
    L.conv1_hs = take(4);
    L.conv2_h16 = take(4 * 9 * 2 * 64 * 4);
    L.l0_h = take(int64_t(L.c_last / 32) * 48 * 2 * 64 * 4);
    L.l1_h = take(int64_t(kHidden / 32) * 48 * 2 * 64 * 4);
    L.lstm_hs = take(2 * kGateCols);
    L.conv2_hw = take(4 * 12 * 2 * 64 * 4);
    L.conv2_hws = take(64);
    L.conv3_hw = n_conv == 3 ? take(8 * 24 * 2 * 64 * 4) : -1;
    L.conv3_hws = n_conv == 3 ? take(128) : -1;
    L.range = take(8);
    L.total = o;
    return L;
}

// conv weight [Cout][Cin][3][3] (torch) -> MFMA 32x32x2 B-operand order:
// out[(nt*KS + (c*3+dy)*3+dx)*64 + lane] = W[32*nt + (lane&31)][2*c + (lane>>5)][dy][dx],  KS = Cin/2*9
static void pack_conv_b_operand(const float* w, int cout, int cin, float* out) {
    const int ks = cin / 2 * 9;
    for (int nt = 0; nt < cout / 32; ++nt)
        for (int c = 0; c < cin / 2; ++c)
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int co = 32 * nt + (lane & 31), ci = 2 * c + (lane >> 5);
                        out[(int64_t(nt) * ks + (c * 3 + dy) * 3 + dx) * 64 + lane] = w[((co * cin + ci) * 3 + dy) * 3 + dx];
                    }
}

// Split precision: every OUTPUT CHANNEL (row of the weight matrix) carries its own power-of-two scale, W' = W * 2^S with
// max |W'| of the row in [2^12, 2^13), W' ~= hi + lo (two f16).  The scale of a row is a per-lane constant of the MFMA's
// D layout (lane & 15 = output channel), so it costs nothing in the kernels and makes the split as good as fp32 for any
// finite weights: an element keeps 22 significant bits unless it is more than 2^16 times smaller than the largest
// weight of ITS OWN row, where its absolute error (2^-37 of that largest weight) is below what fp32 accumulation of the
// row's dot product loses anyway.  The exponent is clamped to what 2^S and 2^-S can hold as normal floats.
static int scale_exp(float wmax) {
    if (!(wmax > 0.f) || !std::isfinite(wmax)) return 0;
    int e = 0;
    (void)std::frexp(wmax, &e);                 // wmax = f * 2^e, f in [0.5, 1)
    int S = 13 - e;                             // wmax * 2^S in [2^12, 2^13)
    return S > 120 ? 120 : (S < -100 ? -100 : S);
}
static void split_f16(double v, uint16_t& hb, uint16_t& lb) {
    const float vf = float(v);
    const _Float16 hi = static_cast<_Float16>(vf);
    const _Float16 lo = static_cast<_Float16>(vf - static_cast<float>(hi));
    std::memcpy(&hb, &hi, 2);
    std::memcpy(&lb, &lo, 2);
}
// max |w| of each of `rows` rows of `len` contiguous weights -> exponents S[r]; descale[r] = 2^-S[r]
static void row_scales(const float* w, int rows, int64_t len, std::vector<int>& S, float* descale) {
    S.resize(rows);
    for (int r = 0; r < rows; ++r) {
        float m = 0.f;
        for (int64_t i = 0; i < len; ++i) m = std::fmax(m, std::fabs(w[r * len + i]));
        S[r] = scale_exp(m);
        descale[r] = std::ldexp(1.0f, -S[r]);
    }
}
// max over rows of sum |w| (the l1 operator bound of a conv layer: |out| <= max|in| * this + max|bias|)
static float max_row_l1(const float* w, int rows, int64_t len) {
    double best = 0.0;
    for (int r = 0; r < rows; ++r) {
        double s = 0.0;
        for (int64_t i = 0; i < len; ++i) s += std::fabs(double(w[r * len + i]));
        best = std::fmax(best, s);
    }
    return float(best * (1.0 + 1e-6));
}
static float max_abs(const float* v, int n) {
    float m = 0.f;
    for (int i = 0; i < n; ++i) m = std::fmax(m, std::fabs(v[i]));
    return m;
}

// conv2 weight [64][32][3][3] -> split-precision f16 B operands for v_mfma_f32_16x16x32_f16.
// k-step ks = dx*3 + dy covers all 32 input channels of tap (dy, dx); lane (n = lane&15, kq = lane>>4) holds
// B[k = 8kq + j][n] = W'[16*nt + n][8kq + j][dy][dx], j = 0..7, as 4 dwords.  descale[64] = 2^-S per output channel.
static void pack_conv2_f16x3(const float* w, float* out_words16, float* descale) {
    std::vector<int> S;
    row_scales(w, 64, 32 * 9, S, descale);
    uint16_t* o16b = reinterpret_cast<uint16_t*>(out_words16);
    for (int nt = 0; nt < 4; ++nt)
        for (int dx = 0; dx < 3; ++dx)
            for (int dy = 0; dy < 3; ++dy) {
                const int ks = dx * 3 + dy;
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int co = 16 * nt + (lane & 15), ci = 8 * (lane >> 4) + j;
                        uint16_t hb, lb;
                        split_f16(std::ldexp(double(w[((co * 32 + ci) * 3 + dy) * 3 + dx]), S[co]), hb, lb);
                        const int64_t base = ((int64_t(nt) * 9 + ks) * 2) * 64 * 8;
                        o16b[base + lane * 8 + j] = hb;
                        o16b[base + 64 * 8 + lane * 8 + j] = lb;
                    }
            }
}

// conv2 weight [64][32][3][3] -> the 1-D Winograd F(2,3) form along the rows (dy), split precision, for cnn2w_kernel:
//   U0 = w[dy=0], U1 = (w0 + w1 + w2)/2, U2 = (w0 - w1 + w2)/2, U3 = w[dy=2]   (per co, ci, dx; computed in double)
// k-step ks = xi*3 + dx covers all 32 input channels; lane (n = lane&15, kq = lane>>4) holds
// B[k = 8kq + j][n] = U_xi[dx][8kq + j][16*nt + n] * 2^S[co].  descale[64] = 2^-S per output channel (over all xi).
// Generalised over (cout, cin): cin / 32 channel blocks cb, k-step ks = (xi*3 + dx) * (cin/32) + cb  (conv3: 24 k-steps).
static void pack_conv_wino_f16x3(const float* w, int cout, int cin, float* out_words, float* descale) {
    std::vector<double> U(size_t(cout) * cin * 4 * 3);          // [co][ci][xi][dx]
    std::vector<int> S(cout);
    const int ncb = cin / 32;
    for (int co = 0; co < cout; ++co) {
        double m = 0.0;
        for (int ci = 0; ci < cin; ++ci)
            for (int dx = 0; dx < 3; ++dx) {
                const double w0 = w[((co * cin + ci) * 3 + 0) * 3 + dx], w1 = w[((co * cin + ci) * 3 + 1) * 3 + dx],
                             w2 = w[((co * cin + ci) * 3 + 2) * 3 + dx];
                double* u = &U[((size_t(co) * cin + ci) * 4) * 3 + dx];
                u[0] = w0;
                u[3] = 0.5 * (w0 + w1 + w2);
                u[6] = 0.5 * (w0 - w1 + w2);
                u[9] = w2;
                for (int xi = 0; xi < 4; ++xi) m = std::fmax(m, std::fabs(u[3 * xi]));
            }
        S[co] = scale_exp(float(m) * 1.0000001f);
        descale[co] = std::ldexp(1.0f, -S[co]);
    }
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out_words);
    for (int nt = 0; nt < cout / 16; ++nt)
        for (int xi = 0; xi < 4; ++xi)
            for (int dx = 0; dx < 3; ++dx)
                for (int cb = 0; cb < ncb; ++cb) {
                    const int ks = (xi * 3 + dx) * ncb + cb;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int co = 16 * nt + (lane & 15), ci = 32 * cb + 8 * (lane >> 4) + j;
                            uint16_t hb, lb;
                            split_f16(std::ldexp(U[((size_t(co) * cin + ci) * 4 + xi) * 3 + dx], S[co]), hb, lb);
                            const int64_t base = ((int64_t(nt) * 12 * ncb + ks) * 2) * 64 * 8;
                            o16[base + lane * 8 + j] = hb;
                            o16[base + 64 * 8 + lane * 8 + j] = lb;
                        }
                }
}

// conv3 weight [128][64][3][3] -> split-precision f16 B operands for v_mfma_f32_16x16x32_f16:
// k-step ks = (cb*3 + dx)*3 + dy covers input channels 32*cb .. 32*cb+31 of tap (dy, dx); lane (n = lane&15, kq = lane>>4)
// holds B[k = 8kq + j][n] = W'[16*nt + n][32*cb + 8kq + j][dy][dx].  descale[128] = 2^-S per output channel.
static void pack_conv3_f16x3(const float* w, float* out_words, float* descale) {
    std::vector<int> S;
    row_scales(w, 128, 64 * 9, S, descale);
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out_words);
    for (int nt = 0; nt < 8; ++nt)
        for (int cb = 0; cb < 2; ++cb)
            for (int dx = 0; dx < 3; ++dx)
                for (int dy = 0; dy < 3; ++dy) {
                    const int ks = (cb * 3 + dx) * 3 + dy;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int co = 16 * nt + (lane & 15), ci = 32 * cb + 8 * (lane >> 4) + j;
                            uint16_t hb, lb;
                            split_f16(std::ldexp(double(w[((co * 64 + ci) * 3 + dy) * 3 + dx]), S[co]), hb, lb);
                            const int64_t base = ((int64_t(nt) * 18 + ks) * 2) * 64 * 8;
                            o16[base + lane * 8 + j] = hb;
                            o16[base + 64 * 8 + lane * 8 + j] = lb;
                        }
                }
}

// conv1 weight [32][1][3][3] as the A operand of v_mfma_f32_32x32x16_f16 (M = channel, K = 9 taps, 7 zero taps):
// lane (m = lane&31, h = lane>>5) holds A[m][k = 8h + j] = w1[c][k] * 2^S[c] for k < 9, else 0,
// where c = (m&3) + 4*(m>>3) + 16*((m>>2)&1): the MFMA's D rows are permuted so that an output lane (which holds rows
// (j&3) + 8*(j>>2) + 4*(lane>>5), j = 0..15) ends up with the 16 CONTIGUOUS channels 16*(lane>>5) + j.
// One scale for the tensor (the kernel's descale is wave-uniform): descale[0] = 2^-S.  The bias is the MFMA's C operand.
static void pack_conv1_f16x3(const float* w, float* out_words, float* descale) {
    std::vector<int> S;
    row_scales(w, 1, 32 * 9, S, descale);
    S.assign(32, S[0]);
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out_words);
    for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
            const int mrow = lane & 31, k = 8 * (lane >> 5) + j;
            const int m = (mrow & 3) + 4 * (mrow >> 3) + 16 * ((mrow >> 2) & 1);
            uint16_t hb, lb;
            split_f16(k < 9 ? std::ldexp(double(w[m * 9 + k]), S[m]) : 0.0, hb, lb);
            o16[lane * 8 + j] = hb;
            o16[64 * 8 + lane * 8 + j] = lb;
        }
}

// weight_ih [4H][K] (gate rows i,f,g,o) -> [K/16][768][16]: for every group of 16 consecutive k and every packed column
// (column = (hb*3 + gate)*32 + u  <-  row goff[gate] + 32*hb + u) the 16 weights ordered by (k mod 4, k div 4),
// so that lane (n, kq) of a 16x16x4 f32 MFMA finds its B values of four consecutive k-steps (k = 4s + kq) in ONE
// 16-byte load and a wave's load covers 1 KiB contiguous.
static void pack_lstm(const float* w_ih, const float* b_ih, const float* b_hh, int K, float* wt, float* b) {
    const int goff[3] = {0, 2 * kHidden, 3 * kHidden};   // i, g, o
    for (int hb = 0; hb < kHidden / 32; ++hb)
        for (int g = 0; g < 3; ++g)
            for (int u = 0; u < 32; ++u) {
                const int col = (hb * 3 + g) * 32 + u, row = goff[g] + 32 * hb + u;
                for (int k = 0; k < K; ++k) {
                    const int kg = k >> 4, kk = k & 15, slot = (kk & 3) * 4 + (kk >> 2);
                    wt[(int64_t(kg) * kGateCols + col) * 16 + slot] = w_ih[int64_t(row) * K + k];
                }
                b[col] = b_ih[row] + b_hh[row];
            }
}

// W_ih [4*hidden][K] -> split-precision f16 B operands for v_mfma_f32_16x16x32_f16, same column order as pack_lstm
// (column c = (hb*3 + gate)*32 + u): k-block kb covers k = 32 kb .. 32 kb + 31, N-tile nt = c / 16; lane (n = lane&15,
// kq = lane>>4) holds B[k = 8 kq + j][n] = W'[row(16 nt + n)][32 kb + 8 kq + j], j = 0..7.  W' = W * 2^S per gate row;
// descale[768] = 2^-S in packed column order.
static void pack_lstm_f16x3(const float* w_ih, int K, float* out_words, float* descale) {
    const int goff[3] = {0, 2 * kHidden, 3 * kHidden};   // i, g, o
    std::vector<int> S(kGateCols);
    for (int c = 0; c < kGateCols; ++c) {
        const int hb = c / 96, g = (c % 96) / 32, u = c % 32, row = goff[g] + 32 * hb + u;
        float m = 0.f;
        for (int k = 0; k < K; ++k) m = std::fmax(m, std::fabs(w_ih[int64_t(row) * K + k]));
        S[c] = scale_exp(m);
        descale[c] = std::ldexp(1.0f, -S[c]);
    }
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out_words);
    for (int kb = 0; kb < K / 32; ++kb)
        for (int nt = 0; nt < kGateCols / 16; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int c = 16 * nt + (lane & 15), hb = c / 96, g = (c % 96) / 32, u = c % 32;
                    const int row = goff[g] + 32 * hb + u, k = 32 * kb + 8 * (lane >> 4) + j;
                    uint16_t hb16, lb16;
                    split_f16(std::ldexp(double(w_ih[int64_t(row) * K + k]), S[c]), hb16, lb16);
                    const int64_t base = ((int64_t(kb) * (kGateCols / 16) + nt) * 2) * 64 * 8;   // in f16 units
                    o16[base + lane * 8 + j] = hb16;
                    o16[base + 64 * 8 + lane * 8 + j] = lb16;
                }
}

}  // namespace ww

using namespace ww;

extern "C" {

int ww_abi_version(void) { return WW_ABI_VERSION; }
const char* ww_last_error(void) { return ww::last_error(); }

int ww_mel_filterbank_host(float* out_host) {
    if (!out_host) return fail(WW_EINVAL, "null output");
    build_mel_filterbank(out_host);
    return WW_OK;
}

int ww_kaiser_best_host(float* out_host) {
    if (!out_host) return fail(WW_EINVAL, "null output pointer");
    build_kaiser_best(out_host);
    return WW_OK;
}

int ww_hann_window_host(float* out_host) {
    if (!out_host) return fail(WW_EINVAL, "null output");
    std::vector<double> w(kNfft);
    build_hann(w.data());
    for (int n = 0; n < kNfft; ++n) out_host[n] = float(w[n]);
    return WW_OK;
}

int64_t ww_packed_weights_floats(int32_t n_conv) {
    if (n_conv != 2 && n_conv != 3) return fail(WW_EINVAL, "n_conv must be 2 or 3, got %d", n_conv);
    return packed_layout(n_conv).total;
}

int ww_pack_weights_host(const ww_state_dict* sd, float* out) {
    if (!sd || !out) return fail(WW_EINVAL, "null argument");
    if (sd->n_conv != 2 && sd->n_conv != 3) return fail(WW_EINVAL, "n_conv must be 2 or 3, got %d", sd->n_conv);
    if (sd->hidden != kHidden) return fail(WW_EUNSUPPORTED, "hidden size %d (only %d is built)", sd->hidden, kHidden);
    for (int i = 0; i < sd->n_conv; ++i)
        if (!sd->conv_weight[i] || !sd->conv_bias[i]) return fail(WW_EINVAL, "conv%d weight/bias missing", i + 1);
    for (int l = 0; l < 2; ++l)
        if (!sd->lstm_weight_ih[l] || !sd->lstm_bias_ih[l] || !sd->lstm_bias_hh[l])
            return fail(WW_EINVAL, "lstm layer %d weight/bias missing", l);
    if (!sd->fc_weight || !sd->fc_bias) return fail(WW_EINVAL, "fc weight/bias missing");

    const PackedLayout L = packed_layout(sd->n_conv);
    std::memset(out, 0, sizeof(float) * L.total);
    std::memcpy(out + L.conv1_w, sd->conv_weight[0], sizeof(float) * 32 * 9);
    std::memcpy(out + L.conv1_b, sd->conv_bias[0], sizeof(float) * 32);
    pack_conv_b_operand(sd->conv_weight[1], 64, 32, out + L.conv2_w);
    std::memcpy(out + L.conv2_b, sd->conv_bias[1], sizeof(float) * 64);
    if (sd->n_conv == 3) {
        pack_conv_b_operand(sd->conv_weight[2], 128, 64, out + L.conv3_w);
        std::memcpy(out + L.conv3_b, sd->conv_bias[2], sizeof(float) * 128);
    }
    pack_lstm(sd->lstm_weight_ih[0], sd->lstm_bias_ih[0], sd->lstm_bias_hh[0], L.c_last, out + L.l0_w, out + L.l0_b);
    pack_lstm(sd->lstm_weight_ih[1], sd->lstm_bias_ih[1], sd->lstm_bias_hh[1], kHidden, out + L.l1_w, out + L.l1_b);
    std::memcpy(out + L.fc_w, sd->fc_weight, sizeof(float) * 2 * kHidden);
    std::memcpy(out + L.fc_b, sd->fc_bias, sizeof(float) * 2);
    if (sd->n_conv == 3) pack_conv3_f16x3(sd->conv_weight[2], out + L.conv3_h, out + L.conv3_hs);
    pack_conv1_f16x3(sd->conv_weight[0], out + L.conv1_h, out + L.conv1_hs);
    pack_conv2_f16x3(sd->conv_weight[1], out + L.conv2_h16, out + L.conv2_hs);
    pack_conv_wino_f16x3(sd->conv_weight[1], 64, 32, out + L.conv2_hw, out + L.conv2_hws);
    if (sd->n_conv == 3) pack_conv_wino_f16x3(sd->conv_weight[2], 128, 64, out + L.conv3_hw, out + L.conv3_hws);
    pack_lstm_f16x3(sd->lstm_weight_ih[0], L.c_last, out + L.l0_h, out + L.lstm_hs);
    pack_lstm_f16x3(sd->lstm_weight_ih[1], kHidden, out + L.l1_h, out + L.lstm_hs + kGateCols);
    // range bounds for the per-clip activation exponents of the f16x3 kernels: |conv_l out| <= max|in| * l1[l] + bmax[l]
    out[L.range + 0] = max_row_l1(sd->conv_weight[0], 32, 9);
    out[L.range + 1] = max_abs(sd->conv_bias[0], 32);
    out[L.range + 2] = max_row_l1(sd->conv_weight[1], 64, 32 * 9);
    out[L.range + 3] = max_abs(sd->conv_bias[1], 64);
    return WW_OK;
}

}  // extern "C"
