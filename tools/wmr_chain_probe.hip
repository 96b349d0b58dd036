// One web-mercator keep flag per thread and nothing else: the body whose ISA tools/wmr_isa_count.py counts (static f64
// operations of the per-point chain of csrc/pcv_wmr_dev.h, compiled with the library's flags).
#include <hip/hip_runtime.h>

#include "../point_cloud_viewer_amd/csrc/pcv_wmr_dev.h"

extern "C" __global__ void wmr_chain_probe(const double* rect, const double* x, const double* y, const double* z, unsigned char* keep) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  keep[i] = wmr::contains(rect, x[i], y[i], z[i]) ? 1 : 0;
}
