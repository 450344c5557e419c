// tests/cpp/decode_window_erasures_demo.cpp — a viewer's crop of a received FIXED frame through include/ternary_codec_v6.hpp, with the
// bytes above 26 of the frame taken as erasures: the coded words are read once, never written, and only the tiles the window covers are
// decoded where the framing allows it.  Host compiler only (g++), links -lt3hip.
//   decode_window_erasures_demo IN.words FW FH X0 Y0 W H OUT.px
//       IN.words: the coded words of one frame as received -> decode_window_erasures -> OUT.px (W * H PixelYCbCrQuant records, row by
//       row; nothing is written when the header does not decode).  Prints one JSON line: the status and the three counts.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ternary_codec_v6.hpp"

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: decode_window_erasures_demo IN.words FW FH X0 Y0 W H OUT.px\n"); return 1; }
    uint32_t g[6];
    for (int i = 0; i < 6; ++i) g[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 10);
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<Word27> words((size_t)bytes / sizeof(Word27));
    if (fread(words.data(), sizeof(Word27), words.size(), f) != words.size()) { fclose(f); return 2; }
    fclose(f);
    DecoderContext dctx; dctx.cfg_last_seen.mode = T3_MODE_FIXED;          // the frame's own header tells the rest
    std::vector<PixelYCbCrQuant> px; ErasureReport rep;
    const bool ok = decode_window_erasures(words, g[0], g[1], g[2], g[3], g[4], g[5], px, dctx, &rep);
    f = fopen(argv[8], "wb"); if (!f) return 2;
    fwrite(px.data(), sizeof(PixelYCbCrQuant), px.size(), f);
    fclose(f);
    printf("{\"ok\": %d, \"status\": %d, \"pixels\": %zu, \"counts\": [%u, %u, %u]}\n", ok ? 1 : 0, t3::last_status(), px.size(), rep.uncorrectable, rep.flagged_blocks,
           rep.flagged_accepted);
    return 0;
}
