// ria_amd/csrc/fallback_relevance.hpp — which codewords of a frame the fallback stage of v2::decodeFixedFrame
// (src/protocol/frame_v2.cpp:1836-1866) can repair the frame through, read from the frame's current bytes.
//
// The fallback substitutes ONE re-decoded codeword at a time, reassembles, verifies and reverts on failure; the
// re-decode has no other effect.  So the re-decodes of codeword c are dead work when no substitution of c alone can make
// the frame verify:
//   * c >= 1 and the header in codeword 0 does not parse: the reassembly is empty whatever c holds;
//   * c >= 1, the header parses, and codewords 0..c-1 already supply all `expected` bytes: reassembleCodewords leaves
//     its loop before reading c, the trial equals the current frame, which is known to be invalid.  What the codewords
//     before c supply does not depend on c (nor does their 0xD5 two-byte marker skip).
// Codeword 0 holds the header, so its re-decodes always matter.
//
// Host and device: recovery_kernels.hip.h reassembles with cws_walk and prunes the fill queue with
// fallback_relevant_cws; tests/helpers/fallback_relevance_check.cpp compiles this file with the host compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RIA_FRAME_HD __host__ __device__
#else
#define RIA_FRAME_HD
#endif

namespace ria {

// The walk of reassembleCodewords (frame_v2.cpp:959-989) over n_cw decoded codewords of bpc bytes for a frame of
// `expected` bytes: take(i, skip, at, n) is called for every codeword i that is read - n bytes from its byte `skip` on (2
// behind the 0xD5 marker of a codeword i != 0, else 0) go to byte `at` of the frame.  first_byte(i): byte 0 of codeword i.
// Returns the frame's length.
template <class FirstByte, class Take>
RIA_FRAME_HD inline int cws_walk(int expected, int n_cw, int bpc, FirstByte first_byte, Take take) {
    int n = 0;
    for (int i = 0; i < n_cw; ++i) {
        const int remaining = expected - n;
        if (remaining == 0) break;
        int skip = 0, avail = bpc;
        if (i != 0 && first_byte(i) == 0xD5) { skip = 2; avail -= 2; }
        const int c = remaining < avail ? remaining : avail;
        take(i, skip, n, c);
        n += c;
    }
    return n;
}
// bytes of a frame whose header parsed (parseHeader, frame_v2.cpp:1195-1252): control 20, data 17 + payload + 2
RIA_FRAME_HD inline int frame_expected_bytes(bool ctl, int plen) { return ctl ? 20 : 17 + plen + 2; }

// cw: the four current codewords, codeword c at cw + c * stride (bpc bytes each); hdr_ok / ctl / plen: parseHeader of
// codeword 0.  Bit c of the result: a substitution of codeword c alone can change a verifying trial.
RIA_FRAME_HD inline unsigned fallback_relevant_cws(const uint8_t* cw, int stride, int bpc, bool hdr_ok, bool ctl, int plen) {
    unsigned mask = 1u;
    if (!hdr_ok) return mask;
    cws_walk(frame_expected_bytes(ctl, plen), 4, bpc, [&](int i) { return cw[i * stride]; },
             [&](int i, int, int, int) { mask |= 1u << i; });
    return mask;
}

}  // namespace ria
