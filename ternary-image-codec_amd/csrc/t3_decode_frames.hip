// t3_decode_frames.hip — the fused FIXED pixel decoder (t3_decode_px.h) over a batch of equal frames in one launch: the kernels
// dec_frames_kernel() (t3_api_decode.cpp) picks from -- one k on all bands, 1-D, no beacon, pixels or RGB out.  Built, like
// t3_decode_fused.hip, without the compiler's atomic optimiser (the ticket draw).
#include "t3_decode_px.h"

namespace t3 {

#define T3_INST_FRAMES(R) template __global__ void dec_frames_px<R, false, false>(const DecFramesArgs); template __global__ void dec_frames_px<R, true, false>(const DecFramesArgs);
T3_INST_FRAMES(2) T3_INST_FRAMES(4) T3_INST_FRAMES(6) T3_INST_FRAMES(8)

}  // namespace t3
