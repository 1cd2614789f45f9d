// ials_tile.h -- the one number the diagonal-tile code (ials_diag.cuh, also built alone by scripts/micro/diag_tile.hip) shares with
// the host plan of an IALS half-step (ials_plan.h, also built alone by g++): no HIP in here.
#pragma once

namespace mi355rec {

constexpr int TP = 17;                   // padded row length of a 16 x 16 tile staged in LDS (conflict-free operand reads)

}  // namespace mi355rec
