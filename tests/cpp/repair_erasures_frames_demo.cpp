// tests/cpp/repair_erasures_frames_demo.cpp — a relay's loop over a file of N equal FIXED frames through include/ternary_codec_v6.hpp,
// with the bytes above 26 of the received frames taken as erasures: the frames are read back to back into one vector, repaired in place
// by ONE repair_erasures_frames call -- corrected codewords on the wire, no pixels -- and forwarded.  Host compiler only (g++), links
// -lt3hip.
//   repair_erasures_frames_demo IN.words N OUT.words
//       IN.words: the coded words of N frames of one size as received -> repair_erasures_frames -> OUT.words (what is forwarded: a block
//       beyond repair travels on as it came, a frame whose header does not decode unchanged).  Prints one JSON line: per frame its
//       status and the six counts.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ternary_codec_v6.hpp"

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: repair_erasures_frames_demo IN.words N OUT.words\n"); return 1; }
    const size_t n_frames = (size_t)strtoul(argv[2], nullptr, 10);
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<Word27> words((size_t)bytes / sizeof(Word27));
    if (fread(words.data(), sizeof(Word27), words.size(), f) != words.size()) { fclose(f); return 2; }
    fclose(f);
    DecoderContext dctx; dctx.cfg_last_seen.mode = T3_MODE_FIXED;          // the frames' own headers tell the rest
    std::vector<ErasureReport> reps; std::vector<int> status;
    const bool ok = repair_erasures_frames(words, n_frames, dctx, &reps, EncoderConfig{}.superframe_words, &status);
    f = fopen(argv[3], "wb"); if (!f) return 2;
    fwrite(words.data(), sizeof(Word27), words.size(), f);
    fclose(f);
    printf("{\"ok\": %d, \"status\": %d, \"frames\": [", ok ? 1 : 0, t3::last_status());
    for (size_t i = 0; i < reps.size(); ++i)
        printf("%s[%d, %u, %u, %u, %u, %u, %u]", i ? ", " : "", status[i], reps[i].header_rewritten, reps[i].uncorrectable, reps[i].blocks_changed, reps[i].bytes_changed,
               reps[i].flagged_blocks, reps[i].flagged_accepted);
    printf("]}\n");
    return 0;
}
