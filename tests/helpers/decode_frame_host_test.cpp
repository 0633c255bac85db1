// Drives ria_host::decodeFrame (ria_amd/host/gpu_waveform.hpp) over rows of soft bits, one row per call on one handle, the way
// gui::StreamingDecoder hands each frame's soft bits to decodeFrame.  Built with g++ against the C ABI only.
//   decode_frame_host_test <modulation> <code_rate> <use_channel_interleave> <rows.f32> <stride> <n_llr.i32> <out.bin>
// out.bin: per row the 32-byte ria_dframe_result, then success, codewords_ok, codewords_failed, frame_type, frame_data size
// (five int32) and frame_data zero-padded to `stride / 648 (at least 4) * bytes_per_codeword` bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ria_amd/host/gpu_waveform.hpp"

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int mod = atoi(argv[1]), rate = atoi(argv[2]), ch = atoi(argv[3]), stride = atoi(argv[5]);
    ria_host::GpuHandle gpu(static_cast<ria_host::Modulation>(mod), static_cast<ria_host::CodeRate>(rate));
    FILE* fr = fopen(argv[4], "rb");
    FILE* fn = fopen(argv[6], "rb");
    FILE* fo = fopen(argv[7], "wb");
    if (!fr || !fn || !fo) return 3;
    const size_t cap = static_cast<size_t>(stride / 648 > 4 ? stride / 648 : 4) * gpu.geo().bytes_per_codeword;
    std::vector<float> row(static_cast<size_t>(stride));
    int32_t n = 0;
    int rows = 0;
    while (fread(&n, sizeof(n), 1, fn) == 1 && fread(row.data(), sizeof(float), row.size(), fr) == row.size()) {
        std::vector<float> soft(row.begin(), row.begin() + (n < 0 ? 0 : n > stride ? stride : n));
        const ria_host::DecodeFrameResult r = ria_host::decodeFrame(gpu, soft, ch != 0);
        const int32_t head[5] = {r.success ? 1 : 0, r.codewords_ok, r.codewords_failed, r.frame_type, static_cast<int32_t>(r.frame_data.size())};
        std::vector<uint8_t> bytes(cap, 0);
        if (r.frame_data.size() > cap) return 4;
        for (size_t i = 0; i < r.frame_data.size(); ++i) bytes[i] = r.frame_data[i];
        fwrite(&r.detail, sizeof(r.detail), 1, fo);
        fwrite(head, sizeof(head), 1, fo);
        fwrite(bytes.data(), 1, bytes.size(), fo);
        ++rows;
    }
    fclose(fo);
    printf("%d\n", rows);
    return 0;
}
