// t3_enc_plan.hpp — the encoder's tile planner (t3_enc_plan.cpp): the tile, LDS carve-up and arguments of one K2 launch.
// Pure C++17, no device: the launch side (t3_api_encode.cpp) adds the tables' addresses, the kernel and what depends on the stream.
#pragma once
#include <stdint.h>

#include "t3_device.h"
#include "t3_host.hpp"

namespace t3 {

enum class EncKind { MfmaK, Uep, Lut };     // matrix cores: one k on all nine bands / bands grouped by k (UEP); LUT fallback
// One K2 launch.  Its arguments lack only what depends on the stream: the tile tickets, and body_out when the beacon pass follows.
struct EncLaunch { EncArgs a; const void* fn; uint32_t block; EncKind kind; };

// One launch of `kind` over the bands of band_mask: tile, LDS carve-up, arguments; false when no tile fits (out.a zeroed).  The tables
// enter as their byte size and the offset of every k's part in them (k index order; t3_api_encode.cpp: the LUT caches).
bool plan_enc_group(const t3_layout& L, const t3_cfg& cfg, uint32_t band_mask, int fe, uint32_t lut_bytes, const uint32_t k_off[4], EncKind kind, EncLaunch& out);

}  // namespace t3
