// Host check of ria_amd/csrc/fallback_relevance.hpp (tests/test_fallback_relevance_host.py): the codewords the rule calls
// irrelevant cannot change the fallback's trial frame, the ones it calls relevant can.  Reassembly and verification are
// restated here on their own (the stripped codewords concatenated and cut to the expected length; a bitwise CRC), so the
// walk the rule shares with the kernels is checked against something that is not itself.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../ria_amd/csrc/fallback_relevance.hpp"

namespace {

uint16_t crc16(const uint8_t* d, int n) {   // CRC-16/CCITT-FALSE
    uint16_t crc = 0xFFFF;
    for (int i = 0; i < n; ++i) {
        crc ^= static_cast<uint16_t>(d[i]) << 8;
        for (int j = 0; j < 8; ++j) crc = (crc & 0x8000) ? static_cast<uint16_t>((crc << 1) ^ 0x1021) : static_cast<uint16_t>(crc << 1);
    }
    return crc;
}
const int kControl[8] = {0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40};
bool is_control(int t) { for (int c : kControl) if (c == t) return true; return false; }

bool parse_header(const uint8_t* d, int len, bool* ctl, int* plen) {
    if (len < 20 || d[0] != 0x55 || d[1] != 0x4C) return false;
    *ctl = is_control(d[2]);
    if (*ctl) { *plen = 0; return crc16(d, 18) == ((d[18] << 8) | d[19]); }
    *plen = (d[13] << 8) | d[14];
    return crc16(d, 15) == ((d[15] << 8) | d[16]);
}
struct Frame { uint8_t cw[4][68]; };
// the trial frame of four codewords: empty when the header in codeword 0 does not parse
std::vector<uint8_t> reassemble(const Frame& f, int bpc) {
    bool ctl; int plen;
    if (!parse_header(f.cw[0], bpc, &ctl, &plen)) return {};
    std::vector<uint8_t> all;
    for (int i = 0; i < 4; ++i) {
        const int skip = (i != 0 && f.cw[i][0] == 0xD5) ? 2 : 0;
        all.insert(all.end(), f.cw[i] + skip, f.cw[i] + bpc);
    }
    const size_t expected = ctl ? 20 : 17 + plen + 2;
    if (all.size() > expected) all.resize(expected);
    return all;
}
bool verify(const std::vector<uint8_t>& d) {
    bool ctl; int plen;
    const int len = static_cast<int>(d.size());
    if (len == 0 || !parse_header(d.data(), len, &ctl, &plen)) return false;
    if (ctl) return true;
    const int sz = 17 + plen + 2;
    return len >= sz && crc16(d.data(), sz - 2) == ((d[sz - 2] << 8) | d[sz - 1]);
}
unsigned rule(const Frame& f, int bpc) {
    bool ctl = false; int plen = 0;
    const bool hdr = parse_header(f.cw[0], bpc, &ctl, &plen);
    return ria::fallback_relevant_cws(&f.cw[0][0], 68, bpc, hdr, ctl, plen);
}

std::mt19937 rng(20261004u);
uint8_t rnd() { return static_cast<uint8_t>(rng() & 0xFF); }

// the bytes of `frame` laid into four codewords; marker bit i: codeword i (1..3) starts with the 0xD5 marker and a filler
// byte.  false if a codeword without the marker would start with 0xD5 by chance (the caller draws another frame).
bool lay_out(const std::vector<uint8_t>& frame, int bpc, int markers, Frame* out) {
    size_t n = 0;
    for (int i = 0; i < 4; ++i) {
        for (int b = 0; b < 68; ++b) out->cw[i][b] = b < bpc ? rnd() : 0;
        int off = 0;
        if (i != 0 && ((markers >> i) & 1)) { out->cw[i][0] = 0xD5; off = 2; }
        const size_t c = std::min(frame.size() - n, static_cast<size_t>(bpc - off));
        std::memcpy(out->cw[i] + off, frame.data() + n, c);
        n += c;
        if (i != 0 && off == 0 && out->cw[i][0] == 0xD5) { if (c > 0) return false; out->cw[i][0] = 0x5D; }
    }
    return true;
}
std::vector<uint8_t> make_frame(int type, int plen) {
    std::vector<uint8_t> f(is_control(type) ? 20 : 17 + plen + 2);
    for (auto& b : f) b = rnd();
    f[0] = 0x55; f[1] = 0x4C; f[2] = static_cast<uint8_t>(type);
    if (is_control(type)) {
        const uint16_t c = crc16(f.data(), 18);
        f[18] = c >> 8; f[19] = c & 0xFF;
    } else {
        f[13] = plen >> 8; f[14] = plen & 0xFF;
        const uint16_t h = crc16(f.data(), 15);
        f[15] = h >> 8; f[16] = h & 0xFF;
        const uint16_t c = crc16(f.data(), 17 + plen);
        f[17 + plen] = c >> 8; f[18 + plen] = c & 0xFF;
    }
    return f;
}

long n_frames = 0, n_relevant = 0, n_irrelevant = 0, n_fail = 0;
void fail(const char* what, int bpc, int type, int plen, int hv, int markers, int c) {
    if (++n_fail <= 20) std::printf("FAIL %s: bpc %d type 0x%02x plen %d header variant %d markers %d codeword %d\n", what, bpc, type, plen, hv, markers, c);
}

// hv: 0 header valid, 1 wrong magic, 2 wrong header CRC (a control frame's is its 18-byte CRC).  want: the mask the rule must
// give, or -1 where this program states none
void check(int bpc, int type, int plen, int hv, int markers, int want) {
    Frame good, cur;
    std::vector<uint8_t> frame;
again:
    do frame = make_frame(type, plen); while (!lay_out(frame, bpc, markers, &good));
    // the frame as the fallback meets it: the frame check fails (a data frame's stored CRC is wrong), the header as `hv` says
    std::vector<uint8_t> bad = frame;
    if (!is_control(type)) bad[bad.size() - 1] ^= 0x04;
    if (hv == 1) bad[1] ^= 0x10;
    if (hv == 2) bad[is_control(type) ? 19 : 16] ^= 0x01;
    cur = good;                       // same filler and markers, only the frame's bytes differ
    {
        size_t n = 0;
        for (int i = 0; i < 4; ++i) {
            const int off = (i != 0 && ((markers >> i) & 1)) ? 2 : 0;
            const size_t c = std::min(bad.size() - n, static_cast<size_t>(bpc - off));
            std::memcpy(cur.cw[i] + off, bad.data() + n, c);
            n += c;
            if (i != 0 && off == 0 && cur.cw[i][0] == 0xD5) goto again;   // the corrupted byte became a marker by chance
        }
    }
    ++n_frames;
    const unsigned mask = rule(cur, bpc);
    if (want >= 0 && mask != static_cast<unsigned>(want)) fail("mask", bpc, type, plen, hv, markers, static_cast<int>(mask));
    if (!(mask & 1u)) fail("codeword 0 dropped", bpc, type, plen, hv, markers, 0);
    const std::vector<uint8_t> trial0 = reassemble(cur, bpc);
    const bool valid0 = verify(trial0);
    const std::vector<uint8_t> tail(frame.end() - std::min<size_t>(frame.size(), bpc), frame.end());
    for (int c = 0; c < 4; ++c) {
        const bool relevant = (mask >> c) & 1u;
        (relevant ? n_relevant : n_irrelevant)++;
        bool changed = false;
        for (int r = 0; r < 66; ++r) {
            Frame t = cur;
            if (r == 64) {
                std::memcpy(t.cw[c], good.cw[c], bpc);    // the codeword as it was sent: the right frame CRC if this codeword holds it
            } else if (r == 65) {
                std::memset(t.cw[c], 0, bpc);             // the end of the sent frame, right CRC included, at the codeword's start
                std::memcpy(t.cw[c], tail.data(), tail.size());
            } else {
                for (int b = 0; b < bpc; ++b) t.cw[c][b] = rnd();
                if (c != 0 && (r & 3) == 0) t.cw[c][0] = 0xD5;
            }
            const std::vector<uint8_t> trial = reassemble(t, bpc);
            if (trial != trial0) changed = true;
            if (!relevant) {
                if (!trial.empty() && trial != trial0) fail("an irrelevant codeword changed the trial", bpc, type, plen, hv, markers, c);
                if (!valid0 && verify(trial)) fail("an irrelevant codeword made the frame verify", bpc, type, plen, hv, markers, c);
            }
        }
        if (relevant && !changed) fail("no replacement of a relevant codeword changed the trial", bpc, type, plen, hv, markers, c);
    }
}

}  // namespace

int main() {
    for (int bpc : {20, 40, 67}) {
        const int largest = 4 * bpc - 19;
        const int plens[8] = {0, 1, bpc - 19, bpc - 18, 2 * bpc - 19, largest, largest + 1, largest + 300};
        for (int hv = 0; hv < 3; ++hv)
            for (int markers = 0; markers < 16; markers += 2) {
                for (int t : kControl) check(bpc, t, 0, hv, markers, 1);   // 20 bytes, all in codeword 0, valid header or not
                for (int plen : plens) {
                    // what the header's length says about the codewords read, where it is plain: 17 + plen + 2 bytes, codeword 0
                    // gives bpc of them, codeword 1 gives bpc, or bpc - 2 behind a marker
                    int want = -1;
                    if (hv != 0) want = 1;
                    else if (plen <= bpc - 19) want = 1;
                    else if (plen == bpc - 18) want = 3;
                    else if (plen == 2 * bpc - 19) want = (markers & 2) ? 7 : 3;
                    else want = 15;
                    check(bpc, 0x01, plen, hv, markers, want);
                }
            }
    }
    std::printf("frames %ld relevant %ld irrelevant %ld failures %ld\n", n_frames, n_relevant, n_irrelevant, n_fail);
    return n_fail ? 1 : 0;
}
