// tests/cpp/frames_demo.cpp — a video loop (old/src/main_video_t3v.cpp:24-26: one encode per frame) as one batched call each way, through
// the names of include/ternary_codec_v6.hpp: encode_frames / decode_frames over vectors of frames.  Host compiler only (g++), links -lt3hip.
//   frames_demo N_FRAMES N_PX MODE BAD IN.px OUT.words OUT.px
//       IN.px: N_FRAMES * N_PX pixel records (6 bytes each), frame after frame -> encode_frames (RS(26,20) on all bands, MODE 0 COMPAT /
//       1 FIXED) -> OUT.words (the frames' coded words, 9 bytes each, frame after frame); then, with the first 13 body symbols of frame BAD
//       (-1: none) damaged, decode_frames -> OUT.px (the decoded frames, a failed one as zero records).  Prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ternary_codec_v6.hpp"

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: frames_demo N_FRAMES N_PX MODE BAD IN.px OUT.words OUT.px\n"); return 1; }
    const size_t n_frames = (size_t)atol(argv[1]), n_px = (size_t)atol(argv[2]); const int mode = atoi(argv[3]), bad = atoi(argv[4]);
    std::vector<std::vector<PixelYCbCrQuant>> frames(n_frames, std::vector<PixelYCbCrQuant>(n_px));
    FILE* f = fopen(argv[5], "rb"); if (!f) return 2;
    for (auto& fr : frames) if (n_px && fread(fr.data(), sizeof(PixelYCbCrQuant), n_px, f) != n_px) { fclose(f); return 2; }
    fclose(f);
    EncoderContext ectx; ectx.cfg.mode = (uint8_t)mode;
    ectx.cfg.profile = ProfileID::P3_RS26_20; uep_uniform(ectx.cfg.uep, 2);
    std::vector<std::vector<Word27>> coded;
    if (!encode_frames(frames, coded, ectx)) { fprintf(stderr, "encode_frames: %d\n", t3::last_status()); return 3; }
    f = fopen(argv[6], "wb"); if (!f) return 2;
    for (const auto& c : coded) fwrite(c.data(), sizeof(Word27), c.size(), f);
    fclose(f);
    // frames of unequal size are refused
    std::vector<std::vector<PixelYCbCrQuant>> uneven = frames; uneven.back().push_back(PixelYCbCrQuant{});
    std::vector<std::vector<Word27>> none;
    const bool uneven_refused = !encode_frames(uneven, none, ectx) && none.empty();
    const size_t hs = mode ? 90 : 52;                                          // coded header symbols (t3_layout::header_syms)
    if (bad >= 0 && (size_t)bad < coded.size()) {
        uint8_t* s = (uint8_t*)coded[(size_t)bad].data();
        for (size_t i = hs; i < hs + 13 && i < coded[(size_t)bad].size() * 9; ++i) s[i] = (uint8_t)((s[i] + 1) % 27);
    }
    DecoderContext dctx; dctx.cfg_last_seen.mode = (uint8_t)mode;
    std::vector<std::vector<PixelYCbCrQuant>> back; std::vector<bool> good;
    const bool all = decode_frames(coded, back, dctx, &good);
    f = fopen(argv[7], "wb"); if (!f) return 2;
    const std::vector<PixelYCbCrQuant> zeros(2 * ((n_px + 1) / 2));
    for (size_t i = 0; i < back.size(); ++i) { const auto& b = back[i].empty() ? zeros : back[i]; fwrite(b.data(), sizeof(PixelYCbCrQuant), b.size(), f); }
    fclose(f);
    printf("{\"frames\": %zu, \"words\": %zu, \"all\": %d, \"uneven_refused\": %d, \"good\": [", coded.size(), coded.empty() ? (size_t)0 : coded[0].size(), all ? 1 : 0, uneven_refused ? 1 : 0);
    for (size_t i = 0; i < good.size(); ++i) printf("%s%d", i ? ", " : "", good[i] ? 1 : 0);
    printf("], \"seen_profile\": %d}\n", (int)dctx.cfg_last_seen.profile);
    return 0;
}
