// rt_k_count_packed.hip — the counting build of the 4-wide walk in its packed-key form with the stack cull
// (render_philox2_count_packed, rt_kernels.h): what bench.py --full and render_work run for a world whose
// timed launch takes the packed kernels, so that the work per sample they report is the timed kernel's. In a
// unit of its own: the timed kernels' units compile exactly what they compiled without it.
#define RT_PHILOX_OPAQUE_KEY 1
#include "rt_kernels.h"

namespace rt {
const void* philox_kernel_count_packed(const KernelForm& f) {
  if (f.var == kVarSpheres) return (const void*)render_philox2_count_packed<kVarSpheres | F_WIDE | F_COUNT>;
  return (const void*)render_philox2_count_packed<kVarCornell | F_WIDE | F_COUNT>;
}
}  // namespace rt
