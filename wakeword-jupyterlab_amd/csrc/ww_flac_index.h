// FLAC files, host half (included by ww_files.cpp only: the reader's source stays one translation unit, which its ThreadSanitizer test
// builds on its own): the container walk (optional ID3v2 tag, "fLaC", metadata blocks, STREAMINFO) and the frame index (RFC 9639
// sections 8 and 9.1).  No sample is decoded here -- ww_flac.hip does that on the device.  The host's per-byte work is the sync scan
// (memchr for 0xFF) and the CRC-16 of every frame, so that a damaged file is refused (status != 1, `ok` False) before anything
// reaches the GPU, exactly like an unreadable WAV.
//
// A frame header counts only if its CRC-8 verifies, every field agrees with STREAMINFO (channel count, bits per sample, sample rate,
// block size <= STREAMINFO's maximum) and its frame / sample number continues the previous frame's.  A frame ends where the next such
// header starts -- provided the CRC-16 of the bytes before it verifies; otherwise the candidate was a look-alike inside the frame and the
// scan goes on -- or at the end of the file.  The sum of the block sizes is the file's length in sample frames (STREAMINFO's
// total_samples may be 0 and is not used).
#pragma once
#include <cstring>
#include <vector>

#include "ww_internal.h"

namespace ww {

namespace {

struct CrcTables {
    uint8_t c8[256];
    uint16_t c16[8][256];          // slicing-by-8: c16[k][b] = CRC of byte b followed by k zero bytes
    CrcTables() {
        for (int b = 0; b < 256; ++b) {
            unsigned c = unsigned(b);
            for (int i = 0; i < 8; ++i) c = (c & 0x80) ? ((c << 1) ^ 0x07) : (c << 1);
            c8[b] = uint8_t(c);
            unsigned d = unsigned(b) << 8;
            for (int i = 0; i < 8; ++i) d = (d & 0x8000) ? ((d << 1) ^ 0x8005) : (d << 1);
            c16[0][b] = uint16_t(d);
        }
        for (int k = 1; k < 8; ++k)
            for (int b = 0; b < 256; ++b) {
                const unsigned p = c16[k - 1][b];
                c16[k][b] = uint16_t((p << 8) ^ c16[0][p >> 8]);
            }
    }
};
const CrcTables g_crc;

inline uint8_t crc8(const uint8_t* p, int64_t n) {
    uint8_t c = 0;
    for (int64_t i = 0; i < n; ++i) c = g_crc.c8[c ^ p[i]];
    return c;
}

inline unsigned crc16_update(unsigned c, const uint8_t* p, int64_t n) {
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const unsigned b0 = p[i] ^ (c >> 8), b1 = p[i + 1] ^ (c & 0xFF);
        c = g_crc.c16[7][b0] ^ g_crc.c16[6][b1] ^ g_crc.c16[5][p[i + 2]] ^ g_crc.c16[4][p[i + 3]] ^ g_crc.c16[3][p[i + 4]] ^
            g_crc.c16[2][p[i + 5]] ^ g_crc.c16[1][p[i + 6]] ^ g_crc.c16[0][p[i + 7]];
    }
    for (; i < n; ++i) c = ((c << 8) & 0xFFFF) ^ g_crc.c16[0][(c >> 8) ^ p[i]];
    return c;
}

struct Header {
    int block_size, header_len, chan_assign;
    int64_t number;
};

// One frame header at p (n bytes available): 1 if it is a header of this stream (CRC-8 and fields), else 0.
int parse_header(const uint8_t* p, int64_t n, const FlacHead& h, int blocking, Header* f) {
    if (n < 6 || p[0] != 0xFF || (p[1] & 0xFE) != 0xF8 || (p[1] & 1) != blocking) return 0;
    const int bs_code = p[2] >> 4, sr_code = p[2] & 15, ch = p[3] >> 4, ss = (p[3] >> 1) & 7;
    if (bs_code == 0 || sr_code == 15 || ch > 10 || ss == 3 || (p[3] & 1)) return 0;
    // the coded frame number (fixed blocking, <= 31 bits, <= 6 bytes) or sample number (variable, <= 36 bits, <= 7 bytes)
    int64_t pos = 4;
    const unsigned c0 = p[4];
    int extra;
    int64_t v;
    if (c0 < 0x80) { extra = 0; v = c0; }
    else if (c0 >= 0xC0 && c0 < 0xE0) { extra = 1; v = c0 & 0x1F; }
    else if (c0 >= 0xE0 && c0 < 0xF0) { extra = 2; v = c0 & 0x0F; }
    else if (c0 >= 0xF0 && c0 < 0xF8) { extra = 3; v = c0 & 0x07; }
    else if (c0 >= 0xF8 && c0 < 0xFC) { extra = 4; v = c0 & 0x03; }
    else if (c0 >= 0xFC && c0 < 0xFE) { extra = 5; v = c0 & 0x01; }
    else if (c0 == 0xFE) { extra = 6; v = 0; }
    else return 0;
    if (extra > (blocking ? 6 : 5)) return 0;
    ++pos;
    if (pos + extra + 1 > n) return 0;
    for (int i = 0; i < extra; ++i, ++pos) {
        if ((p[pos] & 0xC0) != 0x80) return 0;
        v = (v << 6) | (p[pos] & 0x3F);
    }
    int bs;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576 << (bs_code - 2);
    else if (bs_code == 6) { if (pos + 1 > n) return 0; bs = p[pos] + 1; pos += 1; }
    else if (bs_code == 7) { if (pos + 2 > n) return 0; bs = ((p[pos] << 8) | p[pos + 1]) + 1; pos += 2; }
    else bs = 256 << (bs_code - 8);
    int rate;
    static const int kRates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    if (sr_code == 0) rate = h.sample_rate;
    else if (sr_code < 12) rate = kRates[sr_code];
    else if (sr_code == 12) { if (pos + 1 > n) return 0; rate = p[pos] * 1000; pos += 1; }
    else { if (pos + 2 > n) return 0; rate = ((p[pos] << 8) | p[pos + 1]) * (sr_code == 14 ? 10 : 1); pos += 2; }
    if (pos + 1 > n || crc8(p, pos) != p[pos]) return 0;
    static const int kBits[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    const int bps = ss ? kBits[ss] : h.bps;
    const int channels = ch < 8 ? ch + 1 : 2;
    if (rate != h.sample_rate || bps != h.bps || channels != h.channels || bs > h.max_block) return 0;
    f->block_size = bs; f->header_len = int(pos + 1); f->chan_assign = ch; f->number = v;
    return 1;
}

inline uint32_t be24(const uint8_t* p) { return uint32_t(p[0]) << 16 | uint32_t(p[1]) << 8 | p[2]; }

bool flac_magic(const uint8_t* win, int64_t win_len) {
    return win_len >= 4 && (!std::memcmp(win, "fLaC", 4) || (win_len >= 10 && !std::memcmp(win, "ID3", 3)));
}

int flac_parse_head(int fd, int64_t fsize, const uint8_t* win, int64_t win_len, FlacHead* h) {
    if (!flac_magic(win, win_len)) return WW_WAV_ENOTRIFF;
    int64_t pos = 0;
    if (!std::memcmp(win, "ID3", 3)) {             // ID3v2: 10-byte header, syncsafe size, optional 10-byte footer (as libFLAC skips it)
        const uint8_t* t = win;
        if ((t[6] | t[7] | t[8] | t[9]) & 0x80) return WW_WAV_ENOTRIFF;
        pos = 10 + ((int64_t(t[6]) << 21) | (int64_t(t[7]) << 14) | (int64_t(t[8]) << 7) | t[9]) + ((t[5] & 0x10) ? 10 : 0);
        uint8_t m[4];
        if (pos + 4 > fsize || !fetch(fd, win, win_len, pos, 4, m) || std::memcmp(m, "fLaC", 4)) return WW_WAV_ENOTRIFF;
    }
    pos += 4;
    bool first = true, last = false;
    while (!last) {
        uint8_t b[4];
        if (pos + 4 > fsize || !fetch(fd, win, win_len, pos, 4, b)) return WW_WAV_ECHUNK;
        last = (b[0] & 0x80) != 0;
        const int type = b[0] & 0x7F;
        const int64_t len = be24(b + 1);
        if (type == 127 || first != (type == 0)) return WW_WAV_ECHUNK;          // STREAMINFO comes first, and only once
        if (pos + 4 + len > fsize) return WW_WAV_ECHUNK;
        if (type == 0) {
            uint8_t s[34];
            if (len != 34 || !fetch(fd, win, win_len, pos + 4, 34, s)) return WW_WAV_ECHUNK;
            h->min_block = (s[0] << 8) | s[1];
            h->max_block = (s[2] << 8) | s[3];
            h->sample_rate = int((uint32_t(s[10]) << 12) | (uint32_t(s[11]) << 4) | (s[12] >> 4));
            h->channels = ((s[12] >> 1) & 7) + 1;
            h->bps = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
            h->total_samples = (int64_t(s[13] & 15) << 32) | (int64_t(s[14]) << 24) | (int64_t(s[15]) << 16) | (int64_t(s[16]) << 8) | s[17];
            if (h->min_block < 16 || h->max_block < h->min_block) return WW_WAV_ECHUNK;
        }
        first = false;
        pos += 4 + len;
    }
    h->audio_start = pos;
    if (h->bps < 4 || h->bps > 24 || h->sample_rate < 1000 || h->sample_rate > 384000) return WW_WAV_EFORMAT;   // 32-bit FLAC: refused
    return 1;
}

int flac_index(const uint8_t* a, int64_t len, const FlacHead& h, std::vector<FlacFrame>* frames, int64_t* n_samples) {
    frames->clear();
    if (len < 8) return WW_WAV_ECHUNK;
    const int blocking = a[1] & 1;
    Header cur;
    if (!parse_header(a, len, h, blocking, &cur)) return WW_WAV_ECHUNK;
    const int64_t first_number = cur.number;
    int64_t start = 0, samples = 0;
    for (;;) {
        // the next verified header behind this frame's header (a frame holds at least one subframe byte and the CRC-16)
        unsigned crc = 0;
        int64_t crc_pos = start;
        int64_t q = start + cur.header_len + 3;
        int64_t end = -1;
        Header next;
        const int64_t want = blocking ? samples + cur.block_size + first_number : int64_t(frames->size()) + 1 + first_number;
        while (q + 6 <= len) {
            const void* hit = std::memchr(a + q, 0xFF, size_t(len - q - 5));
            if (!hit) break;
            const int64_t c = static_cast<const uint8_t*>(hit) - a;
            if (parse_header(a + c, len - c, h, blocking, &next) && next.number == want) {
                crc = crc16_update(crc, a + crc_pos, c - 2 - crc_pos);
                crc_pos = c - 2;
                if (crc == ((unsigned(a[c - 2]) << 8) | a[c - 1])) { end = c; break; }
            }
            q = c + 1;
        }
        if (end < 0) {                                     // the last frame runs to the end of the file
            crc = crc16_update(crc, a + crc_pos, len - 2 - crc_pos);
            if (crc != ((unsigned(a[len - 2]) << 8) | a[len - 1])) return WW_WAV_ECHUNK;
            end = len;
        }
        if (end - start > INT32_MAX) return WW_WAV_ECHUNK;
        frames->push_back(FlacFrame{start, samples, int32_t(end - start), cur.header_len, cur.block_size, cur.chan_assign});
        samples += cur.block_size;
        if (end == len) break;
        start = end;
        cur = next;
    }
    *n_samples = samples;
    return 1;
}

}  // namespace
}  // namespace ww
