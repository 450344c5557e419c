// tests/cpp/image_names_demo.cpp — the image front end's reference names (old/include/io_image.hpp:102-124 resize_rgb_nn, :141-144
// pad_even, :237-337 image_to_words_subword / words_to_image_subword in their memory forms) driven through
// include/ternary_codec_v6.hpp.  Host compiler only (g++), links -lt3hip.
//   image_names_demo                                   host part only: pad_even and the geometry of every mode, one line each
//   image_names_demo SUB CENTERED SW SH IN.rgb DW DH OUT.resized OUT.words OUT.rgb
//       IN.rgb (SW x SH RGB8) -> resize_rgb_nn to DW x DH -> OUT.resized; image_to_words_subword -> OUT.words (9 bytes per word);
//       words_to_image_subword at the mode's standard resolution -> OUT.rgb
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ternary_codec_v6.hpp"

static bool read_all(const char* path, std::vector<uint8_t>& v, size_t n) {
    v.resize(n);
    FILE* f = fopen(path, "rb"); if (!f) return false;
    const size_t got = n ? fread(v.data(), 1, n, f) : 0; fclose(f);
    return got == n;
}
static bool write_all(const char* path, const void* p, size_t n) {
    FILE* f = fopen(path, "wb"); if (!f) return false;
    const size_t put = n ? fwrite(p, 1, n, f) : 0; fclose(f);
    return put == n;
}

int main(int argc, char** argv) {
    if (argc < 11) {
        printf("pad_even %d %d %d %d\n", pad_even(0), pad_even(1), pad_even(7680), pad_even(853));
        const SubwordMode modes[5] = {SubwordMode::S27, SubwordMode::S24, SubwordMode::S21, SubwordMode::S18, SubwordMode::S15};
        for (SubwordMode m : modes) for (int centered = 0; centered < 2; ++centered) {
            int g[6] = {0, 0, 0, 0, 0, 0};
            const int rc = t3hip_image_geometry((int)m, centered, &g[0], &g[1], &g[2], &g[3], &g[4], &g[5]);
            const StdRes t = std_res_for(m); const ActiveWindow w = centered_window(m);
            printf("geometry %d %d rc=%d %d %d %d %d %d %d std %d %d win %u %u\n", (int)m, centered, rc, g[0], g[1], g[2], g[3], g[4], g[5], (int)t.w, (int)t.h, w.x0, w.y0);
        }
        return 0;
    }
    const SubwordMode sub = (SubwordMode)atoi(argv[1]); const bool centered = atoi(argv[2]) != 0;
    ImageU8 src; src.w = atoi(argv[3]); src.h = atoi(argv[4]); src.c = 3;
    if (!read_all(argv[5], src.data, (size_t)src.w * (size_t)src.h * 3)) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    ImageU8 small;
    resize_rgb_nn(src, atoi(argv[6]), atoi(argv[7]), small);
    if (!write_all(argv[8], small.data.data(), small.data.size())) return 2;
    std::vector<Word27> words;
    if (!image_to_words_subword(src, sub, centered, words)) { fprintf(stderr, "image_to_words_subword: %d\n", t3::last_status()); return 3; }
    if (!write_all(argv[9], words.data(), words.size() * sizeof(Word27))) return 2;
    const StdRes t = std_res_for(sub);
    ImageU8 back;
    if (!words_to_image_subword(words, sub, t.w, t.h, back)) { fprintf(stderr, "words_to_image_subword: %d\n", t3::last_status()); return 4; }
    if (!write_all(argv[10], back.data.data(), back.data.size())) return 2;
    printf("{\"words\": %zu, \"w\": %d, \"h\": %d}\n", words.size(), back.w, back.h);
    return 0;
}
