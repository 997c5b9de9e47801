// general_shapes.hpp -- the shapes behind launchDcGeneral and launchTranGeneral (kernels.hpp), which choose among
// them in kernels_general.hip.  Included by kernels_general.hip, kernels_packed.hip and kernels_big.hip only.
#pragma once

#include "kernels.hpp"

namespace csim {

hipError_t launchDcPacked(const GenPlan& pl, const GenDcArgs& a, hipStream_t stream);       // packedLanesFor(pl) == 16
hipError_t launchTranPacked(const GenPlan& pl, const GenTranArgs& a, hipStream_t stream);
hipError_t launchDcBig(const GenPlan& pl, const GenDcArgs& a, hipStream_t stream);          // a.scratch required
// a.knownAlts and a.nKnown are not read: the big kernel hands an instance back only at the end of its window
hipError_t launchTranBig(const GenPlan& pl, const GenTranArgs& a, hipStream_t stream);

} // namespace csim
