// tests/cpp/frame_records_demo.cpp — the writer side of a video in batched calls: encode_frames (include/ternary_codec_v6.hpp) ->
// t3hip_frame_records_dev (all records in one pass) -> t3hip_index_assemble -> t3v_write_crc with the records' CRCs (no second pass over
// the payload, include/io_t3p_t3v.hpp) -> t3v_read_frame (which verifies every payload CRC on the device).  Host compiler only (g++),
// links -lt3hip and the HIP runtime (device buffers for the records call).
//   frame_records_demo N_FRAMES N_PX IN.px OUT.t3v OUT.recs
//       IN.px: N_FRAMES * N_PX pixel records (6 bytes each), frame after frame -> FIXED RS(26,20) frames -> OUT.t3v; OUT.recs: the
//       N_FRAMES assembled t3_frame_record (96 bytes each).  Prints one JSON line.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "io_t3p_t3v.hpp"
#include "ternary_codec_v6.hpp"

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: frame_records_demo N_FRAMES N_PX IN.px OUT.t3v OUT.recs\n"); return 1; }
    const size_t n = (size_t)atol(argv[1]), n_px = (size_t)atol(argv[2]);
    std::vector<std::vector<PixelYCbCrQuant>> frames(n, std::vector<PixelYCbCrQuant>(n_px));
    FILE* f = fopen(argv[3], "rb"); if (!f) return 2;
    for (auto& fr : frames) if (n_px && fread(fr.data(), sizeof(PixelYCbCrQuant), n_px, f) != n_px) { fclose(f); return 2; }
    fclose(f);
    EncoderContext ectx; ectx.cfg.mode = T3_MODE_FIXED;
    ectx.cfg.profile = ProfileID::P3_RS26_20; uep_uniform(ectx.cfg.uep, 2);
    std::vector<std::vector<Word27>> coded;
    if (!encode_frames(frames, coded, ectx) || coded.size() != n) { fprintf(stderr, "encode_frames: %d\n", t3::last_status()); return 3; }
    // the coded frames as a device batch (what t3hip_encode_frames_dev leaves): frame i at i * stride
    const uint64_t words = coded[0].size(), stride = (9 * words + 15) & ~15ull;
    const uint64_t scr_bytes = t3hip_frame_records_scratch_bytes(words, (uint32_t)n);
    uint8_t* d_words = nullptr; t3_frame_record* d_recs = nullptr; void* d_scr = nullptr;
    if (hipMalloc((void**)&d_words, stride * n) != hipSuccess || hipMalloc((void**)&d_recs, sizeof(t3_frame_record) * n) != hipSuccess ||
        hipMalloc(&d_scr, scr_bytes) != hipSuccess) return 4;
    for (size_t i = 0; i < n; ++i) if (hipMemcpy(d_words + i * stride, coded[i].data(), 9 * words, hipMemcpyHostToDevice) != hipSuccess) return 4;
    const t3_cfg c = t3::to_pod(ectx.cfg, ectx.cfg.superframe_words);
    const int rc = t3hip_frame_records_dev(d_words, words, stride, (uint32_t)n, 0, 1, &c, d_recs, d_scr, scr_bytes, nullptr);
    if (rc != T3_OK) { fprintf(stderr, "t3hip_frame_records_dev: %d\n", rc); return 5; }
    std::vector<t3_frame_record> recs(n);
    if (hipMemcpy(recs.data(), d_recs, sizeof(t3_frame_record) * n, hipMemcpyDeviceToHost) != hipSuccess) return 4;   // (waits for the null stream)
    (void)hipFree(d_words); (void)hipFree(d_recs); (void)hipFree(d_scr);
    const uint64_t first_payload = 26 + 20 * n;                                // T3V6 front matter without meta, then the index
    if (t3hip_index_assemble(recs.data(), n, first_payload) != T3_OK) return 5;
    std::vector<uint32_t> crcs(n);
    for (size_t i = 0; i < n; ++i) crcs[i] = recs[i].crc32;
    std::string err;
    if (!T3Container::t3v_write_crc(argv[4], SubwordMode::S27, 854, 480, coded, crcs, "", {}, &err)) { fprintf(stderr, "t3v_write_crc: %s\n", err.c_str()); return 6; }
    f = fopen(argv[5], "wb"); if (!f) return 2;
    fwrite(recs.data(), sizeof(t3_frame_record), n, f); fclose(f);
    size_t read_ok = 0;
    for (size_t i = 0; i < n; ++i) {
        std::vector<Word27> back;
        if (T3Container::t3v_read_frame(argv[4], i, nullptr, back, &err) && back.size() == words && memcmp(back.data(), coded[i].data(), 9 * words) == 0) ++read_ok;
        else fprintf(stderr, "t3v_read_frame %zu: %s\n", i, err.c_str());
    }
    printf("{\"frames\": %zu, \"words\": %llu, \"read_ok\": %zu}\n", n, (unsigned long long)words, read_ok);
    return 0;
}
