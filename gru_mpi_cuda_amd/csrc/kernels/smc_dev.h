// Device helpers of the sequential-Monte-Carlo selection, shared by its two homes: smc_select_f32_kernel
// (smc.hip, a launch per char) and the selection inside gen_persist_smc_kernel (gen_persist_smc.hip, a whole
// call per launch).  Both translation units see the same text, so a value computed by one is the other's
// bit for bit.
#pragma once
#include "common.h"
#include "gen_sample.h"

namespace gk {

namespace {
constexpr int kDead = 0, kLive = 1, kFin = 2;   // SmcSelectArgs::state values (BeamSelectArgs')

DEV float smc_unit(unsigned word) { return (float)(2u * (word >> 9) + 1u) * 0x1p-24f; }   // exact, in [2^-24, 1 - 2^-24]
}  // namespace

}  // namespace gk
