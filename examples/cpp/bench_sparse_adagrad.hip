// One-process timing of the fused Adagrad step (csrc/sparse_table.hip)
// against the launches it replaces in a fused sparse round, the
// scatter-add and the gather of csrc/kernels.hip, on the same buffers.
// Links kernels.hip and sparse_table.hip only: no cluster, no Python.
//
//   build/bench_sparse_adagrad [--rounds N] [--opt lazy_adam|rowwise_lazy_adam] [--bf16]
//                              [--row-len L]
//
// Shape: the sparse bench config, a 1M x 64 fp32 table with 8192 unique
// rows per step; --row-len sets another row length, a multiple of 8. Two key schedules: "hot", the same 8192 rows every step
// (what the bench does: the rows stay in cache), and "rotating", 64
// disjoint sets of 8192 rows taken in turn (128 MiB of table rows between
// two visits of a set). Every round times, each between its own pair of
// HIP events and in alternation:
//   fused   SparseAdagrad, row-wise, with out     (one launch)
//   pair    SparseScatterAdd + SparseGather       (two launches)
// With --opt the rounds time instead, in the same alternation:
//   adam    SparseLazyAdam of that variant, with out (one launch)
//   adagrad SparseAdagrad, row-wise, with out        (one launch)
// With --bf16 the rounds time three pairs, the bf16-table kernel
// (stochastic rounding) beside its fp32 sibling on the same
// keys, gradients, state and out, the sibling's set half a turn away:
//   adagrad / adagrad16   row-wise Adagrad step with out
//   adam / adam16         row-wise lazy Adam step with out
//   gather / gather16     SparseGather over the fp32 / the bf16 table
// and after each bf16-table kernel its 16-bit-wire sibling (adagrad16w,
// adam16w, gather16w: bf16 gradient in, bf16 rows out) on the same keys.
// Output: median, 10th and 90th percentile of each in microseconds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../csrc/kernels.h"

#define CHECK(x)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

namespace {

constexpr size_t kRows = 1u << 20, kHot = 8192, kSets = 64;
size_t g_row_len = 64;  // --row-len

__global__ void fill_kernel(float* p, size_t n, unsigned salt, float scale) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n; i += stride) {
    unsigned x = (static_cast<unsigned>(i) + salt) * 2654435761u;
    x ^= x >> 15;
    p[i] = scale * static_cast<float>(static_cast<int>(x & 0xffffu) - 32768) / 32768.0f;
  }
}

// the upper halves of n floats: bf16 bits, truncated
__global__ void narrow_kernel(uint16_t* dst, const float* src, size_t n) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n; i += stride) dst[i] = static_cast<uint16_t>(__float_as_uint(src[i]) >> 16);
}

// fresh lazy-Adam records of rec floats: p1 = p2 = 1, the rest +0.0
__global__ void fresh_kernel(float* p, size_t n, size_t rec) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n; i += stride) p[i] = i % rec < 2 ? 1.f : 0.f;
}

namespace k = xps::kern;

// the calls' descriptions: kHot rows at keys, an fp32 or a bf16 array
k::SparseRows Rows(const uint64_t* keys, size_t nrows = kHot) {
  return {keys, nrows, g_row_len, 0, 0, kRows};
}
k::SparseTable F32(float* p) { return {p, k::SparseDtype::kF32}; }
k::SparseTable Bf16(uint16_t* p, uint64_t seed) {
  return {p, k::SparseDtype::kBf16, k::Bf16Rounding::kStochastic, seed};
}
k::SparseWire Wire(float* p) { return {p, k::SparseDtype::kF32}; }
k::SparseWire Wire(uint16_t* p) { return {p, k::SparseDtype::kBf16}; }
const k::AdagradParams kAdagrad{0.01f, 1e-8f, /*rowwise=*/true};
k::LazyAdamParams Adam(bool rowwise) { return {0.01f, 0.9f, 0.999f, 1e-8f, rowwise}; }

void Report(const char* schedule, const char* name, std::vector<float>* us) {
  std::sort(us->begin(), us->end());
  size_t n = us->size();
  printf("%-9s %-10s %9.2f %9.2f %9.2f\n", schedule, name, (*us)[n / 2], (*us)[n / 10],
         (*us)[n * 9 / 10]);
}

// microseconds of the launches fn() makes, between two events on the null stream
template <class Fn>
float TimeUs(hipEvent_t e0, hipEvent_t e1, Fn fn) {
  float ms = 0;
  CHECK(hipEventRecord(e0, nullptr));
  fn();
  CHECK(hipEventRecord(e1, nullptr));
  CHECK(hipEventSynchronize(e1));
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  return ms * 1000.f;
}

// --opt: the lazy-Adam launch against the row-wise Adagrad launch, both with
// out, on the same table, gradients and keys; Adagrad visits the set half a
// turn away, as the pair does in the default mode
void AdamRounds(bool rowwise, int rounds, float* table, float* state, float* grad, float* out,
                const uint64_t* keys, hipEvent_t e0, hipEvent_t e1) {
  size_t nstate = k::SparseLazyAdamStateFloats(kRows, g_row_len, rowwise);
  float* records;
  CHECK(hipMalloc(reinterpret_cast<void**>(&records), nstate * 4));
  hipLaunchKernelGGL(fresh_kernel, dim3(4096), dim3(256), 0, nullptr, records, nstate,
                     nstate / kRows);
  CHECK(hipDeviceSynchronize());
  for (int rotating = 0; rotating < 2; ++rotating) {
    std::vector<float> us_adam, us_adagrad;
    for (int r = -20; r < rounds; ++r) {
      size_t turn = static_cast<size_t>(r + 20);
      const uint64_t* k = keys + (rotating ? (turn % kSets) * kHot : 0);
      float us = TimeUs(e0, e1, [&] {
        k::SparseLazyAdam(F32(table), records, Rows(k), Wire(grad), Wire(out), Adam(rowwise));
      });
      if (r >= 0) us_adam.push_back(us);
      if (rotating) k = keys + ((turn + kSets / 2) % kSets) * kHot;
      us = TimeUs(e0, e1, [&] {
        k::SparseAdagrad(F32(table), state, Rows(k), Wire(grad), Wire(out), kAdagrad);
      });
      if (r >= 0) us_adagrad.push_back(us);
    }
    CHECK(hipGetLastError());
    Report(rotating ? "rotating" : "hot", "adam", &us_adam);
    Report(rotating ? "rotating" : "hot", "adagrad", &us_adagrad);
  }
  CHECK(hipFree(records));
}

// --bf16: each bf16-table kernel beside its fp32 sibling and its 16-bit-wire
// sibling. Both tables see the same keys; the lazy-Adam launches share one
// set of records and the Adagrad launches one state, which only the timing
// reads. The 16-bit wire reads the gradient's upper halves and writes out16.
void Bf16Rounds(int rounds, float* table, float* state, float* grad, float* out,
                const uint64_t* keys, hipEvent_t e0, hipEvent_t e1) {
  size_t nstate = k::SparseLazyAdamStateFloats(kRows, g_row_len, true);
  float* records;
  uint16_t *table16, *grad16, *out16;
  CHECK(hipMalloc(reinterpret_cast<void**>(&records), nstate * 4));
  CHECK(hipMalloc(reinterpret_cast<void**>(&table16), kRows * g_row_len * 2));
  CHECK(hipMalloc(reinterpret_cast<void**>(&grad16), kHot * g_row_len * 2));
  CHECK(hipMalloc(reinterpret_cast<void**>(&out16), kHot * g_row_len * 2));
  hipLaunchKernelGGL(narrow_kernel, dim3(64), dim3(256), 0, nullptr, grad16, grad,
                     kHot * g_row_len);
  hipLaunchKernelGGL(fresh_kernel, dim3(4096), dim3(256), 0, nullptr, records, nstate,
                     nstate / kRows);
  // the bf16 table starts as the fp32 table, rounded to nearest
  std::vector<uint64_t> h(kRows);
  for (size_t i = 0; i < kRows; ++i) h[i] = i;
  uint64_t* all;
  CHECK(hipMalloc(reinterpret_cast<void**>(&all), kRows * 8));
  CHECK(hipMemcpy(all, h.data(), kRows * 8, hipMemcpyHostToDevice));
  k::SparseScatterAssign(Bf16(table16, 0), Rows(all, kRows), Wire(table));
  CHECK(hipDeviceSynchronize());
  CHECK(hipFree(all));
  for (int rotating = 0; rotating < 2; ++rotating) {
    std::vector<float> us[9];
    for (int r = -20; r < rounds; ++r) {
      size_t turn = static_cast<size_t>(r + 20);
      const uint64_t* kf = keys + (rotating ? ((turn + kSets / 2) % kSets) * kHot : 0);
      const uint64_t* kb = keys + (rotating ? (turn % kSets) * kHot : 0);
      uint64_t seed = turn;
      float t[9];
      t[0] = TimeUs(e0, e1, [&] {
        k::SparseAdagrad(F32(table), state, Rows(kf), Wire(grad), Wire(out), kAdagrad);
      });
      t[1] = TimeUs(e0, e1, [&] {
        k::SparseAdagrad(Bf16(table16, seed), state, Rows(kb), Wire(grad), Wire(out), kAdagrad);
      });
      t[2] = TimeUs(e0, e1, [&] {
        k::SparseAdagrad(Bf16(table16, seed), state, Rows(kb), Wire(grad16), Wire(out16),
                         kAdagrad);
      });
      t[3] = TimeUs(e0, e1, [&] {
        k::SparseLazyAdam(F32(table), records, Rows(kf), Wire(grad), Wire(out), Adam(true));
      });
      t[4] = TimeUs(e0, e1, [&] {
        k::SparseLazyAdam(Bf16(table16, seed), records, Rows(kb), Wire(grad), Wire(out),
                          Adam(true));
      });
      t[5] = TimeUs(e0, e1, [&] {
        k::SparseLazyAdam(Bf16(table16, seed), records, Rows(kb), Wire(grad16), Wire(out16),
                          Adam(true));
      });
      t[6] = TimeUs(e0, e1, [&] {
        k::SparseGather(F32(table), Rows(kf), Wire(out));
      });
      t[7] = TimeUs(e0, e1, [&] {
        k::SparseGather(Bf16(table16, 0), Rows(kb), Wire(out));
      });
      t[8] = TimeUs(e0, e1, [&] {
        k::SparseGather(Bf16(table16, 0), Rows(kb), Wire(out16));
      });
      for (int i = 0; i < 9 && r >= 0; ++i) us[i].push_back(t[i]);
    }
    CHECK(hipGetLastError());
    const char* names[9] = {"adagrad", "adagrad16", "adagrad16w", "adam",     "adam16",
                            "adam16w", "gather",    "gather16",   "gather16w"};
    for (int i = 0; i < 9; ++i) Report(rotating ? "rotating" : "hot", names[i], &us[i]);
  }
  CHECK(hipFree(records));
  CHECK(hipFree(table16));
  CHECK(hipFree(grad16));
  CHECK(hipFree(out16));
}

}  // namespace

int main(int argc, char** argv) {
  int rounds = 500;
  const char* opt = nullptr;  // none: the default comparison
  bool bf16 = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--rounds") && i + 1 < argc) {
      rounds = atoi(argv[++i]);
    } else if (!strcmp(argv[i], "--opt") && i + 1 < argc &&
               (!strcmp(argv[i + 1], "lazy_adam") || !strcmp(argv[i + 1], "rowwise_lazy_adam"))) {
      opt = argv[++i];
    } else if (!strcmp(argv[i], "--bf16")) {
      bf16 = true;
    } else if (!strcmp(argv[i], "--row-len") && i + 1 < argc) {
      g_row_len = static_cast<size_t>(atoi(argv[++i]));
    } else {
      fprintf(stderr,
              "usage: %s [--rounds N] [--opt lazy_adam|rowwise_lazy_adam] [--bf16] [--row-len L]\n",
              argv[0]);
      return 2;
    }
  }
  if (rounds < 10 || g_row_len == 0 || g_row_len % 8 || g_row_len > 4096) return 2;

  float *table, *state, *grad, *out;
  uint64_t* keys;
  CHECK(hipMalloc(reinterpret_cast<void**>(&table), kRows * g_row_len * 4));
  CHECK(hipMalloc(reinterpret_cast<void**>(&state), kRows * 4));
  CHECK(hipMalloc(reinterpret_cast<void**>(&grad), kHot * g_row_len * 4));
  CHECK(hipMalloc(reinterpret_cast<void**>(&out), kHot * g_row_len * 4));
  CHECK(hipMalloc(reinterpret_cast<void**>(&keys), kSets * kHot * 8));
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, nullptr, table, kRows * g_row_len, 1u,
                     1.0f);
  hipLaunchKernelGGL(fill_kernel, dim3(64), dim3(256), 0, nullptr, grad, kHot * g_row_len, 2u, 1e-3f);
  CHECK(hipMemset(state, 0, kRows * 4));
  // an odd multiplier permutes the 2^20 rows: the sets are disjoint and
  // every row of a set is unique
  std::vector<uint64_t> h(kSets * kHot);
  for (size_t i = 0; i < h.size(); ++i) h[i] = (i * 668265261u + 12345u) & (kRows - 1);
  CHECK(hipMemcpy(keys, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  CHECK(hipDeviceSynchronize());

  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  printf("# %zu x %zu table, %zu rows per step, %d rounds, microseconds\n", kRows, g_row_len, kHot,
         rounds);
  printf("%-9s %-10s %9s %9s %9s\n", "schedule", "kernel", "median", "p10", "p90");
  if (bf16) {
    Bf16Rounds(rounds, table, state, grad, out, keys, e0, e1);
    return 0;
  }
  if (opt) {
    AdamRounds(!strcmp(opt, "rowwise_lazy_adam"), rounds, table, state, grad, out, keys, e0, e1);
    return 0;
  }
  for (int rotating = 0; rotating < 2; ++rotating) {
    std::vector<float> us_fused, us_pair;
    for (int r = -20; r < rounds; ++r) {
      const uint64_t* k = keys + (rotating ? (static_cast<size_t>(r + 20) % kSets) * kHot : 0);
      float ms = 0;
      CHECK(hipEventRecord(e0, nullptr));
      xps::kern::SparseAdagrad(F32(table), state, Rows(k), Wire(grad), Wire(out), kAdagrad);
      CHECK(hipEventRecord(e1, nullptr));
      CHECK(hipEventSynchronize(e1));
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) us_fused.push_back(ms * 1000.f);
      // the pair visits the set half a turn away, as cold as the fused
      // launch found its own
      if (rotating) k = keys + (static_cast<size_t>(r + 20 + kSets / 2) % kSets) * kHot;
      CHECK(hipEventRecord(e0, nullptr));
      xps::kern::SparseScatterAdd(F32(table), Rows(k), Wire(grad));
      xps::kern::SparseGather(F32(table), Rows(k), Wire(out));
      CHECK(hipEventRecord(e1, nullptr));
      CHECK(hipEventSynchronize(e1));
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) us_pair.push_back(ms * 1000.f);
    }
    CHECK(hipGetLastError());
    Report(rotating ? "rotating" : "hot", "fused", &us_fused);
    Report(rotating ? "rotating" : "hot", "pair", &us_pair);
  }
  return 0;
}
