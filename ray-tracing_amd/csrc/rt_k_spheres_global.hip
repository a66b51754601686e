// rt_k_spheres_global.hip — the spheres-only variant's 4-wide kernel that reads the tree from global memory
// (worlds whose tree does not fit the LDS: config 5), in a unit of its own so that it is built without the
// opaque Philox key that the spheres unit sets (RT_PHILOX_OPAQUE_KEY, rt_device.h: C5 +0.5 % with it). The
// kernels live in an anonymous namespace, so each unit's instantiations are its own.
#include "rt_kernels.h"

namespace rt {
template <unsigned V>
const void* global_kernel(int w) {
  return by_waves<1, 2, 3, 4>(w, [](auto W) { return (const void*)render_philox2<V, W()>; });
}
const void* philox_kernel_spheres_global(const KernelForm& f) {
  return f.skip ? global_kernel<kVarSpheres | F_WIDE | F_SKIP>(f.waves) : global_kernel<kVarSpheres | F_WIDE>(f.waves);
}
}  // namespace rt
