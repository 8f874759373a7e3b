// The host half of the split JPEG decode: marker parser + Huffman (entropy) decoder.  Plain C++, no HIP: the two entries call no hip*
// function and initialise no GPU, so DataLoader worker processes call them and stay outside the count of GPU-holding processes.
// They are re-entrant: no global state, the error text goes into the caller's buffer.  The device half (dequantise, IDCT, upsample,
// colour) is csrc/jpeg.hip; the contract of both is in include/dvid_hip.h.
//
// Accepted: SOF0 (baseline, 8-bit, Huffman), one interleaved scan, one component or three in YCbCr with luma 1x1 / 2x1 / 2x2 and chroma
// 1x1, 8-bit quantisation tables, any Huffman tables, DRI / RSTn, stuffed FF 00.  Everything else a decoder could legally meet is
// DVID_ERR_UNSUPPORTED (the caller falls back to a full host decoder); malformed data is DVID_ERR_ARG.  Every read of the input goes
// through a bounds check against [data, data + size): a corrupt file gives an error or wrong coefficients, never a read outside.
//
// The entropy decoder is table-driven: a 64-bit bit buffer refilled 4 bytes at a time while no FF lies in the next 8 (byte by byte through
// stuffing and markers), a 9-bit lookahead table per Huffman table that yields (symbol, length) in one step, and for AC codes whose
// magnitude bits fit the same 9 bits a second table that yields (run, value, length) in one step; longer codes walk the canonical maxcode
// ladder from 10 bits.
// DC prediction and the sign extension of the magnitude bits run in unsigned arithmetic and wrap: corrupt data has no undefined behaviour.
//
// This file also compiles stand-alone (tools/jpeg_entropy_check.cpp builds it with the host compiler under -fsanitize=address,undefined).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/dvid_hip.h"

namespace {

constexpr int kLook = 9;          // lookahead bits

const unsigned char kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Err {
    char* buf;
    int cap;
    int fail(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
        if (buf && cap > 0) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, (size_t)cap, fmt, ap);
            va_end(ap);
        }
        return code;
    }
};

struct HuffTable {
    bool defined = false;
    unsigned char bits[17];          // codes of each length 1..16
    unsigned char vals[256];
    int nvals = 0;
    // derived
    uint16_t look[1 << kLook];          // (length << 8) | symbol for codes of at most kLook bits, 0: longer or absent
    int32_t maxcode[18];                 // largest code of length l, -1: none
    int32_t valoff[17];                  // index of the first value of length l minus its first code
    int maxsym = 0;
    // AC tables: where a code and its magnitude bits fit the lookahead together, (value << 16) | (run << 8) | bits consumed; else 0
    int32_t fast_ac[1 << kLook];
};

// canonical code assignment (ITU T.81 annex C); false when the counts overflow the code space
bool build_table(HuffTable& t) {
    int code = 0, k = 0;
    memset(t.look, 0, sizeof(t.look));
    t.maxsym = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = t.bits[l];
        if (code + n > (1 << l)) return false;
        t.valoff[l] = k - code;
        if (n) {
            for (int i = 0; i < n; ++i, ++code, ++k) {
                if (t.vals[k] > t.maxsym) t.maxsym = t.vals[k];
                if (l <= kLook) {
                    const int first = code << (kLook - l), count = 1 << (kLook - l);
                    const uint16_t e = (uint16_t)((l << 8) | t.vals[k]);
                    for (int j = 0; j < count; ++j) t.look[first + j] = e;
                }
            }
            t.maxcode[l] = code - 1;
        } else {
            t.maxcode[l] = -1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    for (int i = 0; i < (1 << kLook); ++i) {
        t.fast_ac[i] = 0;
        const unsigned e = t.look[i];
        const int len = (int)(e >> 8), run = (int)(e & 255) >> 4, mag = (int)(e & 15);
        if (e && mag && len + mag <= kLook) {
            int v = (i >> (kLook - len - mag)) & ((1 << mag) - 1);
            if (v < (1 << (mag - 1))) v -= (1 << mag) - 1;
            t.fast_ac[i] = (int32_t)(((uint32_t)v << 16) | (uint32_t)(run << 8) | (uint32_t)(len + mag));
        }
    }
    return true;
}

struct Frame {
    dvid_jpeg_info info;
    HuffTable dc[4], ac[4];
    int dc_id[3], ac_id[3];
    int restart = 0;          // MCUs per restart interval, 0: none
    int64_t scan = 0;         // first byte of the entropy-coded data
};

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

const char* sof_name(int m) {
    switch (m) {
        case 0xC1: return "extended sequential (SOF1)";
        case 0xC2: return "progressive (SOF2)";
        case 0xC3: return "lossless (SOF3)";
        case 0xC9: return "arithmetic coding (SOF9)";
        case 0xCA: return "progressive with arithmetic coding (SOF10)";
        default: return m >= 0xC9 ? "arithmetic coding / differential" : "differential";
    }
}

int parse(const uint8_t* d, int64_t size, Frame& f, Err& e) {
    if (!d || size < 4 || d[0] != 0xFF || d[1] != 0xD8) return e.fail(DVID_ERR_ARG, "jpeg: no SOI marker at the start of %lld bytes", (long long)size);
    dvid_jpeg_info& in = f.info;
    memset(&in, 0, sizeof(in));
    uint16_t qt[4][64];
    bool have_qt[4] = {false, false, false, false}, have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1, comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1};
    int64_t p = 2;
    for (;;) {
        if (p + 2 > size) return e.fail(DVID_ERR_ARG, "jpeg: the file ends at byte %lld before a scan", (long long)size);
        if (d[p] != 0xFF) return e.fail(DVID_ERR_ARG, "jpeg: byte %lld is 0x%02X where a marker is expected", (long long)p, d[p]);
        while (p + 1 < size && d[p + 1] == 0xFF) ++p;          // fill bytes
        if (p + 2 > size) return e.fail(DVID_ERR_ARG, "jpeg: the file ends inside a marker");
        const int m = d[p + 1];
        p += 2;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;          // stand-alone markers
        if (m == 0xD9) return e.fail(DVID_ERR_ARG, "jpeg: EOI before any scan");
        if (p + 2 > size) return e.fail(DVID_ERR_ARG, "jpeg: the length field of marker 0x%02X lies past the end", m);
        const int len = rd16(d + p);
        if (len < 2 || p + len > size)
            return e.fail(DVID_ERR_ARG, "jpeg: marker 0x%02X at byte %lld has length %d, the file has %lld bytes left", m, (long long)p - 2, len, (long long)(size - p));
        const uint8_t* s = d + p + 2;
        const int n = len - 2;
        if (m == 0xE0) {
            if (n >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && !memcmp(s, "Adobe", 5)) adobe = true, adobe_transform = s[11];
        } else if (m == 0xDB) {
            int q = 0;
            while (q < n) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq > 1 || tq > 3) return e.fail(DVID_ERR_ARG, "jpeg: DQT with precision %d, table %d", pq, tq);
                if (pq == 1) return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: 16-bit quantisation table %d is not supported", tq);
                if (q + 65 > n) return e.fail(DVID_ERR_ARG, "jpeg: DQT table %d runs past its marker", tq);
                for (int i = 0; i < 64; ++i) qt[tq][kNatural[i]] = s[q + 1 + i];
                have_qt[tq] = true;
                q += 65;
            }
        } else if (m == 0xC4) {
            int q = 0;
            while (q < n) {
                if (q + 17 > n) return e.fail(DVID_ERR_ARG, "jpeg: DHT runs past its marker");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return e.fail(DVID_ERR_ARG, "jpeg: DHT with class %d, table %d", tc, th);
                HuffTable& t = tc ? f.ac[th] : f.dc[th];
                int total = 0;
                t.bits[0] = 0;
                for (int i = 1; i <= 16; ++i) total += (t.bits[i] = s[q + i]);
                if (total > 256 || q + 17 + total > n) return e.fail(DVID_ERR_ARG, "jpeg: DHT table %d lists %d symbols", th, total);
                memcpy(t.vals, s + q + 17, (size_t)total);
                t.nvals = total;
                if (!build_table(t)) return e.fail(DVID_ERR_ARG, "jpeg: the code lengths of DHT table %d overflow the code space", th);
                t.defined = true;
                q += 17 + total;
            }
        } else if (m == 0xC0) {
            if (have_sof) return e.fail(DVID_ERR_ARG, "jpeg: a second SOF marker");
            if (n < 6) return e.fail(DVID_ERR_ARG, "jpeg: SOF0 of %d bytes", n);
            const int prec = s[0], h = rd16(s + 1), w = rd16(s + 3), nc = s[5];
            if (prec != 8) return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: %d-bit samples are not supported (8-bit only)", prec);
            if (h == 0) return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: height 0 (set by a DNL marker) is not supported");
            if (w == 0) return e.fail(DVID_ERR_ARG, "jpeg: width 0");
            if (nc != 1 && nc != 3) return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: %d components are not supported (1, or 3 in YCbCr)", nc);
            if (n < 6 + 3 * nc) return e.fail(DVID_ERR_ARG, "jpeg: SOF0 is too short for %d components", nc);
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = s[6 + 3 * c];
                hs[c] = s[7 + 3 * c] >> 4;
                vs[c] = s[7 + 3 * c] & 15;
                comp_tq[c] = s[8 + 3 * c];
                if (hs[c] < 1 || hs[c] > 4 || vs[c] < 1 || vs[c] > 4 || comp_tq[c] > 3)
                    return e.fail(DVID_ERR_ARG, "jpeg: component %d has sampling %dx%d, table %d", c, hs[c], vs[c], comp_tq[c]);
            }
            in.width = w, in.height = h, in.ncomp = nc;
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC8 && m != 0xCC) {          // the other SOFn (C4 = DHT is handled above; CC = DAC below)
            return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: %s is not supported (baseline SOF0 only)", sof_name(m));
        } else if (m == 0xCC) {
            return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: arithmetic coding (DAC) is not supported");
        } else if (m == 0xDC) {
            return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: a DNL marker is not supported");
        } else if (m == 0xDD) {
            if (n < 2) return e.fail(DVID_ERR_ARG, "jpeg: DRI of %d bytes", n);
            f.restart = rd16(s);
        } else if (m == 0xDA) {
            if (!have_sof) return e.fail(DVID_ERR_ARG, "jpeg: SOS before SOF");
            if (n < 1) return e.fail(DVID_ERR_ARG, "jpeg: empty SOS");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n < 1 + 2 * ns + 3) return e.fail(DVID_ERR_ARG, "jpeg: SOS with %d components in %d bytes", ns, n);
            if (ns != in.ncomp)
                return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: several scans are not supported (the first scan holds %d of %d components)", ns, in.ncomp);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != comp_id[c])
                    return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: the scan lists its components in another order than the frame");
                f.dc_id[c] = s[2 + 2 * c] >> 4;
                f.ac_id[c] = s[2 + 2 * c] & 15;
                if (f.dc_id[c] > 3 || f.ac_id[c] > 3) return e.fail(DVID_ERR_ARG, "jpeg: component %d names Huffman tables %d / %d", c, f.dc_id[c], f.ac_id[c]);
                if (!f.dc[f.dc_id[c]].defined || !f.ac[f.ac_id[c]].defined)
                    return e.fail(DVID_ERR_ARG, "jpeg: component %d uses Huffman table DC %d / AC %d, which is missing", c, f.dc_id[c], f.ac_id[c]);
                if (f.dc[f.dc_id[c]].maxsym > 15) return e.fail(DVID_ERR_ARG, "jpeg: DC table %d holds a category above 15", f.dc_id[c]);
                if (!have_qt[comp_tq[c]]) return e.fail(DVID_ERR_ARG, "jpeg: component %d uses quantisation table %d, which is missing", c, comp_tq[c]);
            }
            const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahl = s[3 + 2 * ns];
            if (ss != 0 || se != 63 || ahl != 0)
                return e.fail(DVID_ERR_ARG, "jpeg: a baseline scan with spectral selection %d..%d, approximation 0x%02X", ss, se, ahl);
            f.scan = p + len;
            break;
        }
        p += len;
    }
    // colour space and sampling
    if (in.ncomp == 3) {
        if (!jfif) {
            if (adobe) {
                if (adobe_transform != 1)
                    return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: Adobe transform %d is not supported (1 = YCbCr only)", adobe_transform);
            } else if (!(comp_id[0] == 1 && comp_id[1] == 2 && comp_id[2] == 3)) {
                return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: no JFIF or Adobe marker and component ids %d, %d, %d: not known to be YCbCr", comp_id[0], comp_id[1], comp_id[2]);
            }
        }
        const bool luma_ok = (hs[0] == 1 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 2);
        if (!luma_ok || hs[1] != 1 || vs[1] != 1 || hs[2] != 1 || vs[2] != 1)
            return e.fail(DVID_ERR_UNSUPPORTED, "jpeg: sampling factors %dx%d, %dx%d, %dx%d are not supported (luma 1x1, 2x1 or 2x2 with chroma 1x1)", hs[0],
                          vs[0], hs[1], vs[1], hs[2], vs[2]);
    } else {
        hs[0] = vs[0] = 1;          // a single component is not interleaved: its MCU is one block whatever the factors say
    }
    const int hmax = hs[0], vmax = vs[0];
    const int mcus_w = (in.width + 8 * hmax - 1) / (8 * hmax), mcus_h = (in.height + 8 * vmax - 1) / (8 * vmax);
    int64_t off = 0;
    for (int c = 0; c < in.ncomp; ++c) {
        in.hsamp[c] = hs[c], in.vsamp[c] = vs[c];
        in.blocks_w[c] = mcus_w * hs[c], in.blocks_h[c] = mcus_h * vs[c];
        in.coef_offset[c] = off;
        off += (int64_t)in.blocks_w[c] * in.blocks_h[c] * 64;
        memcpy(in.quant[c], qt[comp_tq[c]], sizeof(qt[0]));
    }
    in.coef_count = off;
    return DVID_OK;
}

// MSB-first bit reader over the entropy-coded segment.  `fake` counts the zero bits fed once the data ran out (end of file, or a marker):
// a block that consumed any of them read past the scan's end.
struct BitReader {
    const uint8_t* d;
    int64_t pos, end;
    uint64_t buf = 0;
    int bits = 0;
    int64_t fake = 0;

    // at least 32 bits in the buffer afterwards: a code (<= 16 bits) and its magnitude bits (<= 15)
    inline void refill() {
        if (bits > 32) return;
        if (pos + 8 <= end) {
            uint64_t x;
            memcpy(&x, d + pos, 8);
            const uint64_t y = ~x;
            if (!((y - 0x0101010101010101ull) & ~y & 0x8080808080808080ull)) {          // no FF among the next 8 bytes: take 4 at once
                x = __builtin_bswap64(x);
                buf = (buf << 32) | (x >> 32);
                bits += 32;
                pos += 4;
                return;
            }
        }
        refill_bytes();
    }
    __attribute__((noinline)) void refill_bytes() {
        while (bits <= 56) {
            unsigned b = 0;
            if (pos < end) {
                b = d[pos];
                if (b == 0xFF) {
                    if (pos + 1 < end && d[pos + 1] == 0) {
                        pos += 2;
                    } else {          // a marker (or the file's last byte): the data ends here
                        b = 0;
                        fake += 8;
                    }
                } else {
                    ++pos;
                }
            } else {
                fake += 8;
            }
            buf = (buf << 8) | b;
            bits += 8;
        }
    }
    inline unsigned peek(int n) const { return (unsigned)((buf >> (bits - n)) & ((1u << n) - 1)); }
    inline void skip(int n) { bits -= n; }
    inline bool overran() const { return bits < fake; }
};

// one Huffman symbol; -1 when the bits match no code.  At least 16 bits are in the buffer on entry.
inline int decode_symbol(BitReader& br, const HuffTable& t) {
    const unsigned e = t.look[br.peek(kLook)];
    if (e) {
        br.skip((int)(e >> 8));
        return (int)(e & 255);
    }
    for (int l = kLook + 1; l <= 16; ++l) {
        const int code = (int)br.peek(l);
        if (code <= t.maxcode[l]) {
            const int idx = t.valoff[l] + code;
            if (idx < 0 || idx >= t.nvals) return -1;
            br.skip(l);
            return t.vals[idx];
        }
    }
    return -1;
}

// the s magnitude bits of a coefficient of category s (1..16), sign-extended (T.81 F.2.2.1 EXTEND) in unsigned arithmetic
inline uint32_t receive_extend(BitReader& br, int s) {
    const uint32_t v = br.peek(s);
    br.skip(s);
    return v < (1u << (s - 1)) ? v - ((1u << s) - 1u) : v;
}

int decode_scan(const uint8_t* d, int64_t size, const Frame& f, int16_t* coef, Err& e) {
    const dvid_jpeg_info& in = f.info;
    const int hmax = in.hsamp[0], vmax = in.vsamp[0];
    const int mcus_w = in.blocks_w[0] / hmax, mcus_h = in.blocks_h[0] / vmax;
    memset(coef, 0, (size_t)in.coef_count * sizeof(int16_t));
    BitReader br{d, f.scan, size};
    uint32_t pred[3] = {0, 0, 0};
    int until_restart = f.restart, next_rst = 0;
    const int64_t total = (int64_t)mcus_w * mcus_h;
    int64_t done = 0;
    for (int my = 0; my < mcus_h; ++my) {
        for (int mx = 0; mx < mcus_w; ++mx, ++done) {
            if (f.restart && until_restart == 0) {
                // the interval is over: drop the padding bits, meet RSTn exactly here
                if (br.bits - br.fake >= 8 || br.overran())
                    return e.fail(DVID_ERR_ARG, "jpeg: restart marker out of place before MCU %lld (data where RST%d is expected)", (long long)done, next_rst);
                int64_t p = br.pos;
                while (p + 1 < size && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
                if (p + 2 > size || d[p] != 0xFF || d[p + 1] != 0xD0 + next_rst)
                    return e.fail(DVID_ERR_ARG, "jpeg: restart marker out of place before MCU %lld (RST%d expected at byte %lld)", (long long)done, next_rst, (long long)p);
                br.pos = p + 2;
                br.buf = 0, br.bits = 0, br.fake = 0;
                next_rst = (next_rst + 1) & 7;
                until_restart = f.restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < in.ncomp; ++c) {
                const HuffTable& dct = f.dc[f.dc_id[c]];
                const HuffTable& act = f.ac[f.ac_id[c]];
                const int hsc = in.hsamp[c], vsc = in.vsamp[c];
                for (int v = 0; v < vsc; ++v) {
                    for (int h = 0; h < hsc; ++h) {
                        int16_t* blk = coef + in.coef_offset[c] + ((int64_t)(my * vsc + v) * in.blocks_w[c] + (mx * hsc + h)) * 64;
                        br.refill();
                        int s = decode_symbol(br, dct);
                        if (s < 0) return e.fail(DVID_ERR_ARG, "jpeg: a Huffman code that does not exist (DC, MCU %lld)", (long long)done);
                        if (s) {
                            br.refill();
                            pred[c] += receive_extend(br, s);
                        }
                        blk[0] = (int16_t)(uint16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            br.refill();
                            const int32_t fa = act.fast_ac[br.peek(kLook)];
                            if (fa) {          // code and magnitude in one step
                                k += (fa >> 8) & 255;
                                if (k > 63) return e.fail(DVID_ERR_ARG, "jpeg: coefficient index %d past 63 (MCU %lld)", k, (long long)done);
                                br.skip(fa & 255);
                                blk[kNatural[k++]] = (int16_t)(fa >> 16);
                                continue;
                            }
                            const int rs = decode_symbol(br, act);
                            if (rs < 0) return e.fail(DVID_ERR_ARG, "jpeg: a Huffman code that does not exist (AC, MCU %lld)", (long long)done);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s) {
                                k += r;
                                if (k > 63) return e.fail(DVID_ERR_ARG, "jpeg: coefficient index %d past 63 (MCU %lld)", k, (long long)done);
                                blk[kNatural[k]] = (int16_t)(uint16_t)receive_extend(br, s);
                                ++k;
                            } else if (r == 15) {
                                k += 16;
                            } else {
                                break;          // EOB
                            }
                        }
                        if (br.overran()) return e.fail(DVID_ERR_ARG, "jpeg: truncated scan: the data ends inside MCU %lld of %lld", (long long)done, (long long)total);
                    }
                }
            }
            if (f.restart) --until_restart;
        }
    }
    return DVID_OK;
}

}  // namespace

extern "C" {

int dvid_jpeg_parse(const void* data, int64_t size, dvid_jpeg_info* info, char* err, int err_cap) {
    Err e{err, err_cap};
    if (err && err_cap > 0) err[0] = 0;
    if (!data || !info || size < 0) return e.fail(DVID_ERR_ARG, "jpeg parse: null pointer or negative size");
    Frame f;
    const int rc = parse(reinterpret_cast<const uint8_t*>(data), size, f, e);
    if (rc == DVID_OK) *info = f.info;
    return rc;
}

int dvid_jpeg_entropy_decode(const void* data, int64_t size, int16_t* coef, int64_t coef_cap, dvid_jpeg_info* info, char* err, int err_cap) {
    Err e{err, err_cap};
    if (err && err_cap > 0) err[0] = 0;
    if (!data || !coef || size < 0) return e.fail(DVID_ERR_ARG, "jpeg entropy decode: null pointer or negative size");
    Frame f;
    const int rc = parse(reinterpret_cast<const uint8_t*>(data), size, f, e);
    if (rc != DVID_OK) return rc;
    if (coef_cap < f.info.coef_count)
        return e.fail(DVID_ERR_ARG, "jpeg entropy decode: the buffer holds %lld coefficients, the %d x %d file has %lld", (long long)coef_cap, f.info.width,
                      f.info.height, (long long)f.info.coef_count);
    if (info) *info = f.info;
    return decode_scan(reinterpret_cast<const uint8_t*>(data), size, f, coef, e);
}

}  // extern "C"
