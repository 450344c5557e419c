// t3_encode_words.hip — the fused encoder (t3_encode.h) for raw Word27 in (2-D: the row-by-row flow only): every kernel enc_kernel() (t3_api_encode.cpp) can pick for this front end.
#include "t3_encode.h"

namespace t3 {

T3_INST_K(FE_WORDS, 0) T3_INST_K(FE_WORDS, 1)

}  // namespace t3
