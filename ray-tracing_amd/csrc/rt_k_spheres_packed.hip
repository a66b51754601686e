// rt_k_spheres_packed.hip — the spheres-only variant's LDS-staged 4-wide kernels in their packed-key form
// (wide_node<F, true>, include/rt_wide.h: configs 1 and 2 and every world whose tree fits the LDS), in a unit
// of their own: compiled among the spheres unit's other kernels the 4-wave kernel (C2) comes out at 100 B/lane
// of scratch and 30 VGPR spills, here at 92 and 28, the key / reference form's figures. With the opaque
// Philox key, as the spheres unit (rt_k_spheres.hip). The kernels live in an anonymous namespace, so each
// unit's instantiations are its own.
#define RT_PHILOX_OPAQUE_KEY 1
// The shading code's fused sincos (rt_device.h): this unit only, so that every build keeps kernels on the
// plain form (the spheres unit's, RTAMD_WIDE=0) to compare against. The other units lost with it.
#define RT_FUSED_SINCOS 1
#include "rt_kernels.h"

namespace rt {
const void* philox_kernel_spheres_packed(const KernelForm& f) {
  return f.skip ? pick_packed<kVarSpheres | F_WIDE | F_SKIP>(f) : pick_packed<kVarSpheres | F_WIDE>(f);
}
}  // namespace rt
