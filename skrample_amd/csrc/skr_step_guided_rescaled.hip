// The rescaled half of the guided step's one-trip kernels (skr_step_guided.hip): guided_kernel_v1<T, K, NOISE, RowForm, true>, 384
// instantiations, compiled beside the unrescaled half instead of behind it.
#include "skr_step_guided_kernel.h"

namespace skr {

void launch_guided_rescaled_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const skr_step_rescale* rs,
                               const uint64_t* seeds, const GuidedLaunch& l, RowForm form, const RowRef& tab, hipStream_t s) {
  launch_guided_v1<true>(p, inputs, out, gd, rs, seeds, l, form, tab, s);
}

}  // namespace skr
