// Drives ria_host::mcdpskWindow (ria_amd/host/gpu_waveform.hpp) over windows in host memory, one window per call on one handle,
// the way gui::StreamingDecoder hands one sync at a time to decodeCurrentFrame().  Built with g++ against the C ABI only.
//   mcdpsk_window_host_test <carriers> <bps> <spreading> <chirp> <connected> <search_len> <window_len> <windows.f32> <params.bin> <out.bin>
// params.bin: per window pending_total_cw, first_avail (uint32), last_decoded_sync (int32).  out.bin: per window the 64-byte
// ria_mcdpsk_window_result, the 64-byte ria_mcdpsk_acq_result, the frame_data size (int32) and frame_data zero-padded to 320 bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ria_amd/host/gpu_waveform.hpp"

int main(int argc, char** argv) {
    if (argc != 11) return 2;
    ria_mcdpsk_config cfg{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), 0};
    const bool chirp = atoi(argv[4]) != 0, connected = atoi(argv[5]) != 0;
    const size_t search_len = static_cast<size_t>(atol(argv[6])), window_len = static_cast<size_t>(atol(argv[7]));
    ria_host::GpuHandle gpu(ria_host::Modulation::DQPSK, ria_host::CodeRate::R1_4);
    FILE* fw = fopen(argv[8], "rb");
    FILE* fp = fopen(argv[9], "rb");
    FILE* fo = fopen(argv[10], "wb");
    if (!fw || !fp || !fo) return 3;
    std::vector<float> w(window_len);
    int32_t p[3];
    int rows = 0;
    while (fread(p, sizeof(p), 1, fp) == 1 && fread(w.data(), sizeof(float), w.size(), fw) == w.size()) {
        const ria_host::McdpskWindowResult r = ria_host::mcdpskWindow(gpu, cfg, w.data(), window_len, search_len, chirp, connected, 0.0f, 0.0f,
                                                                      static_cast<uint32_t>(p[0]), static_cast<uint32_t>(p[1]), p[2]);
        std::vector<uint8_t> bytes(320, 0);
        if (r.frame_data.size() > bytes.size()) return 4;
        for (size_t i = 0; i < r.frame_data.size(); ++i) bytes[i] = r.frame_data[i];
        const int32_t nb = static_cast<int32_t>(r.frame_data.size());
        fwrite(&r.window, sizeof(r.window), 1, fo);
        fwrite(&r.acq, sizeof(r.acq), 1, fo);
        fwrite(&nb, sizeof(nb), 1, fo);
        fwrite(bytes.data(), 1, bytes.size(), fo);
        ++rows;
    }
    fclose(fo);
    printf("%d\n", rows);
    return 0;
}
