// What the descriptor matcher (orb_match.hip) reads of an extractor (orb.hip).
#pragma once
#include <stdint.h>

#include "ctx.hpp"

struct vdo_orb;

namespace vdo {
// The keypoints of an extractor's last extraction as device arrays in output order: n rows of 32 descriptor bytes, the level-0 positions
// vdo_orb_extract returned (bit for bit) and the octaves.  Valid until the extractor's next extraction; null pointers when n == 0.
struct OrbMatchView {
  vdo_ctx* ctx;
  int n;
  const uint8_t* desc;
  const float *x, *y;
  const int32_t* octave;
};
// Makes the view resident: queues K8 on the extractor's stream unless vdo_orb_descriptors has run since the extraction, and the kernel that scales
// the positions unless an earlier call has.  No download, no synchronisation.  VDO_ERR_INVALID between vdo_orb_extract_begin and _end.
int orb_match_view(vdo_orb* o, OrbMatchView* v);
}  // namespace vdo
