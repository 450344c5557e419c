// t3_encode_px.hip — the fused encoder (t3_encode.h) for quantised YCbCr pixels in: every kernel enc_kernel() (t3_api_encode.cpp) can pick for this front end.
#include "t3_encode.h"

namespace t3 {

T3_INST_K(FE_PIXELS, 0) T3_INST_K(FE_PIXELS, 1) T3_INST_K(FE_PIXELS, 2)

}  // namespace t3
