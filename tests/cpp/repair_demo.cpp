// tests/cpp/repair_demo.cpp — a relay's (or an archive scrubber's) step through include/ternary_codec_v6.hpp: a received FIXED frame is
// repaired in place -- corrected codewords on the wire, no pixels -- and forwarded.  Host compiler only (g++), links -lt3hip.
//   repair_demo IN.words OUT.words
//       IN.words: the coded words of one FIXED frame as received -> repair_profile -> OUT.words (what is forwarded: the repaired frame; a
//       block beyond repair travels on as it came, a frame whose header does not decode unchanged).  Prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ternary_codec_v6.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: repair_demo IN.words OUT.words\n"); return 1; }
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<Word27> words((size_t)bytes / sizeof(Word27));
    if (fread(words.data(), sizeof(Word27), words.size(), f) != words.size()) { fclose(f); return 2; }
    fclose(f);
    DecoderContext dctx; dctx.cfg_last_seen.mode = T3_MODE_FIXED;          // the frame's own header tells the rest
    RepairReport rep;
    const bool ok = repair_profile(words, dctx, &rep);
    f = fopen(argv[2], "wb"); if (!f) return 2;
    fwrite(words.data(), sizeof(Word27), words.size(), f);
    fclose(f);
    printf("{\"ok\": %d, \"status\": %d, \"header_rewritten\": %u, \"uncorrectable\": %u, \"blocks_changed\": %u, \"bytes_changed\": %u}\n",
           ok ? 1 : 0, t3::last_status(), rep.header_rewritten, rep.uncorrectable, rep.blocks_changed, rep.bytes_changed);
    return 0;
}
