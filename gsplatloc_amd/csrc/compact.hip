// The scan between the two passes of an ordered compaction (compact_dev.h): one workgroup, any number of counts.
#include "gsloc_internal.h"

namespace gsl {

// Exclusive scan of counts[nb] -> bases[nb], total -> nnz[0].  One workgroup; thread t owns one contiguous chunk.
__global__ __launch_bounds__(256) void k_count_scan(const uint32_t* __restrict__ counts, int nb,
                                                   uint32_t* __restrict__ bases, int32_t* __restrict__ nnz) {
  __shared__ uint32_t part[256];
  const int per = (nb + 255) / 256;
  const int lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
  uint32_t sum = 0;
  for (int b = lo; b < hi; ++b) sum += counts[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int t = 0; t < 256; ++t) {
      uint32_t v = part[t];
      part[t] = run;
      run += v;
    }
    nnz[0] = (int32_t)run;
  }
  __syncthreads();
  uint32_t run = part[threadIdx.x];
  for (int b = lo; b < hi; ++b) {
    bases[b] = run;
    run += counts[b];
  }
}

void launch_count_scan(hipStream_t st, const uint32_t* counts, int nb, uint32_t* bases, int32_t* total) {
  hipLaunchKernelGGL(k_count_scan, dim3(1), dim3(256), 0, st, counts, nb, bases, total);
}

}  // namespace gsl
