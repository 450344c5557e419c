// t3_encode_frames.hip — the fused encoder (t3_encode.h) over a batch of equal frames in one launch: the kernels enc_frames_kernel()
// (t3_api_encode.cpp) picks from -- pixel and RGB input, one k on all bands, 1-D, no beacon.
#include "t3_encode.h"

namespace t3 {

#define T3_INST_FRAMES(FE) template __global__ void enc_frames_k<FE, 2>(const EncFramesArgs); template __global__ void enc_frames_k<FE, 4>(const EncFramesArgs); \
    template __global__ void enc_frames_k<FE, 6>(const EncFramesArgs); template __global__ void enc_frames_k<FE, 8>(const EncFramesArgs);
T3_INST_FRAMES(FE_PIXELS) T3_INST_FRAMES(FE_RGB)

}  // namespace t3
