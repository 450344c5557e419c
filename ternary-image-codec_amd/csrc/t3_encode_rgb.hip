// t3_encode_rgb.hip — the fused encoder (t3_encode.h) for RGB8 in, the image bridge fused into phase 1: every kernel enc_kernel() (t3_api_encode.cpp) can pick for this front end.
#include "t3_encode.h"

namespace t3 {

T3_INST_K(FE_RGB, 0) T3_INST_K(FE_RGB, 1) T3_INST_K(FE_RGB, 2)

}  // namespace t3
