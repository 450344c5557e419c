// tests/cpp/decode_frames_window_erasures_demo.cpp — a viewer's crop out of every frame of a received run of equal FIXED frames through
// include/ternary_codec_v6.hpp, with the bytes above 26 of the frames taken as erasures: the coded words are read once, never written, and
// where the framing allows it one launch decodes only the tiles the window covers, of all frames.  Host compiler only (g++), links -lt3hip.
//   decode_frames_window_erasures_demo IN.words N FW FH X0 Y0 W H OUT.px
//       IN.words: the coded words of N frames back to back as received -> decode_frames_window_erasures -> OUT.px (N windows of W * H
//       PixelYCbCrQuant records, row by row; all zero for a frame whose header does not decode).  Prints one JSON line: per frame the
//       status and the three counts; "ok" says the call itself went through.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ternary_codec_v6.hpp"

int main(int argc, char** argv) {
    if (argc < 10) { fprintf(stderr, "usage: decode_frames_window_erasures_demo IN.words N FW FH X0 Y0 W H OUT.px\n"); return 1; }
    const size_t n_frames = (size_t)strtoul(argv[2], nullptr, 10);
    uint32_t g[6];
    for (int i = 0; i < 6; ++i) g[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<Word27> words((size_t)bytes / sizeof(Word27));
    if (fread(words.data(), sizeof(Word27), words.size(), f) != words.size()) { fclose(f); return 2; }
    fclose(f);
    DecoderContext dctx; dctx.cfg_last_seen.mode = T3_MODE_FIXED;          // the frames' own headers tell the rest
    std::vector<PixelYCbCrQuant> px; std::vector<ErasureReport> reps; std::vector<int> status;
    decode_frames_window_erasures(words, n_frames, g[0], g[1], g[2], g[3], g[4], g[5], px, dctx, &reps, EncoderConfig{}.superframe_words, &status);
    f = fopen(argv[9], "wb"); if (!f) return 2;
    fwrite(px.data(), sizeof(PixelYCbCrQuant), px.size(), f);
    fclose(f);
    printf("{\"ok\": %d, \"frames\": [", px.size() == (size_t)g[4] * g[5] * n_frames ? 1 : 0);
    for (size_t i = 0; i < n_frames; ++i)
        printf("%s{\"status\": %d, \"counts\": [%u, %u, %u]}", i ? ", " : "", status[i], reps[i].uncorrectable, reps[i].flagged_blocks, reps[i].flagged_accepted);
    printf("]}\n");
    return 0;
}
