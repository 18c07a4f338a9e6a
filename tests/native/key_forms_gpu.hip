// tests/native/key_forms_gpu.hip — TEST TOOL, not product code.
//
// The closed forms of dispatch_core.h evaluated ON THE DEVICE, one thread per case:
//   key_forms_gpu <cases.bin> <out.bin>
// reads a table of KeyFormCase (tests/native/key_forms.h; written by tests/key_edge_cases.py), runs
// one plain kernel — loads, arithmetic, stores — and writes a table of KeyFormOut.
// tests/test_key_forms_gpu.py compares every output with integer references.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "key_forms.h"

using namespace ydc;

__global__ void k_key_forms(const KeyFormCase* __restrict__ tab, KeyFormOut* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const KeyFormCase c = tab[i];
  KeyFormOut o;
  key_forms_eval(c, o);
  out[i] = o;
}

#define HIP_OK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e__ = (expr);                                                               \
    if (e__ != hipSuccess) {                                                               \
      std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e__));                     \
      return 2;                                                                            \
    }                                                                                      \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]);
    return 1;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 1;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (bytes <= 0 || bytes % (long)sizeof(KeyFormCase)) {
    std::fprintf(stderr, "%s: %ld bytes is no table of %zu-byte cases\n", argv[1], bytes, sizeof(KeyFormCase));
    return 1;
  }
  const uint32_t n = (uint32_t)(bytes / (long)sizeof(KeyFormCase));
  std::vector<KeyFormCase> tab(n);
  if (std::fread(tab.data(), sizeof(KeyFormCase), n, f) != n) return 1;
  std::fclose(f);
  KeyFormCase* d_tab = nullptr;
  KeyFormOut* d_out = nullptr;
  HIP_OK(hipMalloc(&d_tab, (size_t)n * sizeof(KeyFormCase)));
  HIP_OK(hipMalloc(&d_out, (size_t)n * sizeof(KeyFormOut)));
  HIP_OK(hipMemcpy(d_tab, tab.data(), (size_t)n * sizeof(KeyFormCase), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_out, 0xEE, (size_t)n * sizeof(KeyFormOut)));
  hipLaunchKernelGGL(k_key_forms, dim3((n + 255) / 256), dim3(256), 0, 0, d_tab, d_out, n);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  std::vector<KeyFormOut> out(n);
  HIP_OK(hipMemcpy(out.data(), d_out, (size_t)n * sizeof(KeyFormOut), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_tab));
  HIP_OK(hipFree(d_out));
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(KeyFormOut), n, f) != n) return 1;
  std::fclose(f);
  std::printf("key_forms_gpu: %u cases\n", n);
  return 0;
}
