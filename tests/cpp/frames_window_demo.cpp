// tests/cpp/frames_window_demo.cpp — a video through the image front end as one batched call each way, and a cropper on top of it, through
// the names of include/ternary_codec_v6.hpp: images_to_frames, frames_to_images, decode_frames_window.  Host compiler only (g++), links -lt3hip.
//   frames_window_demo N SW SH BAD X0 Y0 W H IN.rgb OUT.words OUT.rgb OUT.win
//       IN.rgb: N RGB8 images of SW x SH, one after the other -> images_to_frames (S15, not centred: 854 x 480 frames; FIXED, RS(26,20) on
//       all bands) -> OUT.words (the frames' coded words, frame after frame); then, with 13 symbols of body block 0 of frame BAD (-1: none)
//       damaged, frames_to_images -> OUT.rgb (854 x 480 RGB8 per frame, a failed one as zeros) and decode_frames_window of the W x H window at
//       (X0, Y0) -> OUT.win (pixel records, a failed frame as zero records).  Prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ternary_codec_v6.hpp"

int main(int argc, char** argv) {
    if (argc < 13) { fprintf(stderr, "usage: frames_window_demo N SW SH BAD X0 Y0 W H IN.rgb OUT.words OUT.rgb OUT.win\n"); return 1; }
    const size_t n = (size_t)atol(argv[1]); const int sw = atoi(argv[2]), sh = atoi(argv[3]), bad = atoi(argv[4]);
    const int x0 = atoi(argv[5]), y0 = atoi(argv[6]), w = atoi(argv[7]), h = atoi(argv[8]);
    std::vector<ImageU8> images(n);
    FILE* f = fopen(argv[9], "rb"); if (!f) return 2;
    for (auto& im : images) {
        im.w = sw; im.h = sh; im.c = 3; im.data.resize((size_t)sw * (size_t)sh * 3);
        if (fread(im.data.data(), 1, im.data.size(), f) != im.data.size()) { fclose(f); return 2; }
    }
    fclose(f);
    const SubwordMode sub = SubwordMode::S15; const StdRes res = std_res_for(sub);
    EncoderContext ectx; ectx.cfg.mode = T3_MODE_FIXED;
    ectx.cfg.profile = ProfileID::P3_RS26_20; uep_uniform(ectx.cfg.uep, 2);
    std::vector<std::vector<Word27>> coded;
    if (!images_to_frames(images, sub, false, coded, ectx)) { fprintf(stderr, "images_to_frames: %d\n", t3::last_status()); return 3; }
    f = fopen(argv[10], "wb"); if (!f) return 2;
    for (const auto& c : coded) fwrite(c.data(), sizeof(Word27), c.size(), f);
    fclose(f);
    // images of unequal size are refused
    std::vector<ImageU8> uneven = images; uneven.back().w -= 1;
    std::vector<std::vector<Word27>> none;
    const bool uneven_refused = !images_to_frames(uneven, sub, false, none, ectx) && none.empty();
    if (bad >= 0 && (size_t)bad < coded.size()) {
        uint8_t* s = (uint8_t*)coded[(size_t)bad].data();
        for (size_t i = 90; i < 90 + 13 && i < coded[(size_t)bad].size() * 9; ++i) s[i] = (uint8_t)((s[i] + 1) % 27);   // 90: the FIXED header's symbols
    }
    // the decoder knows the stream's configuration (DecoderContext remembers one)
    DecoderContext dctx; dctx.cfg_last_seen.mode = T3_MODE_FIXED;
    dctx.cfg_last_seen.profile = ProfileID::P3_RS26_20; uep_uniform(dctx.cfg_last_seen.uep, 2);
    std::vector<ImageU8> back; std::vector<bool> good_img, good_win;
    const bool all_img = frames_to_images(coded, sub, false, back, dctx, &good_img);
    f = fopen(argv[11], "wb"); if (!f) return 2;
    const std::vector<uint8_t> zeros((size_t)res.w * (size_t)res.h * 3);
    for (const auto& im : back) { const auto& b = im.data.empty() ? zeros : im.data; fwrite(b.data(), 1, b.size(), f); }
    fclose(f);
    std::vector<std::vector<PixelYCbCrQuant>> wins;
    const bool all_win = decode_frames_window(coded, res.w, res.h, x0, y0, w, h, wins, dctx, &good_win);
    f = fopen(argv[12], "wb"); if (!f) return 2;
    const std::vector<PixelYCbCrQuant> zpx((size_t)w * (size_t)h);
    for (const auto& q : wins) { const auto& b = q.empty() ? zpx : q; fwrite(b.data(), sizeof(PixelYCbCrQuant), b.size(), f); }
    fclose(f);
    printf("{\"frames\": %zu, \"words\": %zu, \"uneven_refused\": %d, \"all_img\": %d, \"all_win\": %d, \"good_img\": [", coded.size(), coded.empty() ? (size_t)0 : coded[0].size(),
           uneven_refused ? 1 : 0, all_img ? 1 : 0, all_win ? 1 : 0);
    for (size_t i = 0; i < good_img.size(); ++i) printf("%s%d", i ? ", " : "", good_img[i] ? 1 : 0);
    printf("], \"good_win\": [");
    for (size_t i = 0; i < good_win.size(); ++i) printf("%s%d", i ? ", " : "", good_win[i] ? 1 : 0);
    printf("]}\n");
    return 0;
}
