// pn_step_state.h -- what moving a pn_step_state to the next step means, for the kernels that do it on the device: the
// last workgroup of an optimizer's last launch (pn_train.hip, pn_optim.hip).  Include after <hip/hip_runtime.h>.
#pragma once
#include <cstdint>

#include "../../include/pathnet_hip.h"

namespace pn {
// epoch += 1, adam_step += 1, seed = splitmix64(seed)   (= step_state_advance_kernel, pn_context.hip)
__device__ __forceinline__ void advance_step_state(pn_step_state *s) {
    s->epoch += 1;
    s->adam_step += 1;
    uint64_t z = (s->seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    s->seed = z ^ (z >> 31);
}
}  // namespace pn
