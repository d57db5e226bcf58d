// Device-resident positions of a rolling batch (include/skrample_hip.h, skr_rolling_advance): one thread per slot computes the row
// the slot's sample reads this tick and the timestep its network sees, from state the host validated once at admission, and moves
// the slot on.  The step kernels neither check nor clamp an index (skr_step_launch_rolling); this kernel is the check: an index
// it publishes names a row inside the slot's own run, anything else is -1.  No host-to-device copy per tick, so a tick's network
// can sit in a captured graph behind it.
#include "skr_step_common.h"
#include "skr_device.h"

namespace skr {

__global__ __launch_bounds__(BLOCK) void rolling_advance_kernel(int32_t* __restrict__ position, const int32_t* __restrict__ length,
                                                                const uint32_t* __restrict__ times, int32_t* __restrict__ sample_index,
                                                                uint32_t* __restrict__ timesteps, int32_t capacity, int32_t max_steps) {
  const int32_t b = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
  if (b >= capacity) return;
  const int32_t p = position[b], n = length[b];
  if (p >= 0 && p < n && n <= max_steps) {
    const int32_t row = b * max_steps + p;  // < capacity * max_steps <= INT32_MAX (checked by the entry)
    sample_index[b] = row;
    timesteps[b] = times[row];  // (moved as bits: what the host uploaded is what the network reads)
    position[b] = p + 1;
  } else {
    sample_index[b] = -1;  // free, finished or inconsistent: timesteps[b] and position[b] keep their bytes
  }
}

}  // namespace skr

extern "C" int skr_rolling_advance(int32_t* position_dev, const int32_t* length_dev, const float* times_dev, int32_t* sample_index_dev,
                                   float* timesteps_dev, int32_t capacity, int32_t max_steps, void* stream) {
  using namespace skr;
  if (!position_dev || !length_dev || !times_dev || !sample_index_dev || !timesteps_dev) return SKR_ERR_NULL;
  if (capacity < 1 || max_steps < 1 || (int64_t)capacity * max_steps > INT32_MAX) return SKR_ERR_SHAPE;
  DeviceGuard device_guard(position_dev);
  const unsigned blocks = ((unsigned)capacity + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(rolling_advance_kernel, dim3(blocks), dim3(BLOCK), 0, reinterpret_cast<hipStream_t>(stream), position_dev, length_dev,
                     reinterpret_cast<const uint32_t*>(times_dev), sample_index_dev, reinterpret_cast<uint32_t*>(timesteps_dev), capacity,
                     max_steps);
  return finish_launch();
}
