// One-process sweep of the batched dual write (dst0[i] = dst1[i] = src[i]):
// the shipped kern::BatchedAssign2 against reference rows (1R:1W copy,
// 0R:2W fill, 1R:0W read) and shape variants of one templated kernel, all
// interleaved round-robin in one process, every launch timed with its own
// pair of HIP events. Links kernels.hip only: no cluster, no Python.
//
//   build/bench_dualwrite [--rounds N] [--variants a,b,...] [--segments N]
//                         [--seg-mb N] [--list]
//
// A variant is `runs` or `walk` plus ':'-separated options:
//   runs        block-uniform segment runs (tile_runs.h), uniform pointers
//   walk        the per-lane segment walk (the shape shipped before runs)
//   uN          N loads in flight per lane (1, 2, 4, 8), all issued first
//   g | i       stores grouped per destination | interleaved (default)
//   ntN         nontemporal: 0 none, 1 loads, 2 both stores, 3 all three
//   tN          tile of N KiB per block (default 128)
//   pgN         fixed grid of 256*N blocks looping over tiles (default: one
//               tile per block)
//   rotN        start N chunks * tile index into the tile, wrap around
//   bsN         block size 256, 512, 1024
//   copy | fill | read   reference modes 1R:1W, 0R:2W, 1R:0W
// e.g. --variants ship,runs,runs:u4:g:nt3:t512
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../csrc/kernels.h"
#include "../../csrc/tile_runs.h"

#define CHECK(x)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

namespace {

using xps::kern::kMaxBatch;
using xps::kern::Seg2;
using xps::kern::TileRun;
using xps::kern::TileRunIter;

typedef unsigned int v4 __attribute__((ext_vector_type(4)));

struct SegArr {
  Seg2 d[kMaxBatch];
  unsigned long long prefix[kMaxBatch + 1];
  int n;
};

enum Mode { kDual = 0, kCopy = 1, kFill = 2, kRead = 3 };

template <int NT>
__device__ __forceinline__ v4 Ld(const v4* p) {
  if (NT & 1) return __builtin_nontemporal_load(p);
  return *p;
}
template <int NT>
__device__ __forceinline__ void St(v4* p, v4 v) {
  if (NT & 2) {
    __builtin_nontemporal_store(v, p);
  } else {
    *p = v;
  }
}

// chunks [lo, hi) of one segment, block-uniform pointers and bounds
template <int BS, int U, bool G, int NT, int MODE>
__device__ __forceinline__ void CopyRun(v4* __restrict__ d0, v4* __restrict__ d1,
                                        const v4* __restrict__ sp, size_t lo, size_t hi, v4& acc) {
  size_t i = lo + threadIdx.x;
  if (U > 1) {
    for (; i + static_cast<size_t>(U - 1) * BS < hi; i += static_cast<size_t>(U) * BS) {
      v4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (MODE == kFill) {
          v[u] = acc;
        } else {
          v[u] = Ld<NT>(sp + i + u * BS);
        }
      }
      if (MODE == kRead) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc ^= v[u];
      } else if (G) {
#pragma unroll
        for (int u = 0; u < U; ++u) St<NT>(d0 + i + u * BS, v[u]);
        if (MODE != kCopy) {
#pragma unroll
          for (int u = 0; u < U; ++u) St<NT>(d1 + i + u * BS, v[u]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          St<NT>(d0 + i + u * BS, v[u]);
          if (MODE != kCopy) St<NT>(d1 + i + u * BS, v[u]);
        }
      }
    }
  }
  for (; i < hi; i += BS) {
    v4 v = MODE == kFill ? acc : Ld<NT>(sp + i);
    if (MODE == kRead) {
      acc ^= v;
    } else {
      St<NT>(d0 + i, v);
      if (MODE != kCopy) St<NT>(d1 + i, v);
    }
  }
}

// WALK: every lane walks the segment list itself (one load, two stores,
// no unrolling). Otherwise: block-uniform runs.
template <int BS, bool WALK, int U, bool G, int NT, int MODE>
__global__ __launch_bounds__(BS) void dw_kernel(SegArr da, size_t cpb, size_t ntiles, size_t rot,
                                                v4* sink) {
  const size_t total = da.prefix[da.n];
  v4 acc = {threadIdx.x, blockIdx.x, 3u, 4u};
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    size_t first = tile * cpb;
    size_t end = first + cpb;
    if (end > total) end = total;
    if (first >= end) break;
    if (WALK) {
      int seg = 0;
      {
        int lo = 0, hi = da.n - 1;
        while (lo < hi) {
          int mid = (lo + hi + 1) >> 1;
          if (da.prefix[mid] <= first) {
            lo = mid;
          } else {
            hi = mid - 1;
          }
        }
        seg = lo;
      }
      size_t seg_lo = da.prefix[seg], seg_hi = da.prefix[seg + 1];
      v4* d0 = static_cast<v4*>(da.d[seg].dst0);
      v4* d1 = static_cast<v4*>(da.d[seg].dst1);
      const v4* sp = static_cast<const v4*>(da.d[seg].src);
      for (size_t g = first + threadIdx.x; g < end; g += BS) {
        if (g >= seg_hi) {
          do {
            ++seg;
            seg_hi = da.prefix[seg + 1];
          } while (g >= seg_hi);
          seg_lo = da.prefix[seg];
          d0 = static_cast<v4*>(da.d[seg].dst0);
          d1 = static_cast<v4*>(da.d[seg].dst1);
          sp = static_cast<const v4*>(da.d[seg].src);
        }
        size_t local = g - seg_lo;
        v4 v = sp[local];
        d0[local] = v;
        d1[local] = v;
      }
    } else {
      // rotated start: [first + r, end) then [first, first + r)
      size_t r = rot ? (tile * rot) % (end - first) : 0;
      for (int piece = 0; piece < 2; ++piece) {
        size_t b = piece == 0 ? first + r : first;
        size_t e = piece == 0 ? end : first + r;
        TileRunIter it = xps::kern::TileRunsRange(da.prefix, da.n, b, e);
        TileRun run;
        while (xps::kern::TileRunsNext(da.prefix, &it, &run)) {
          CopyRun<BS, U, G, NT, MODE>(static_cast<v4*>(da.d[run.seg].dst0),
                                      static_cast<v4*>(da.d[run.seg].dst1),
                                      static_cast<const v4*>(da.d[run.seg].src), run.lo, run.hi,
                                      acc);
        }
      }
    }
  }
  if (MODE == kRead && (acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x5eedf00du) sink[0] = acc;
}

struct Shape {
  int bs = 256, u = 1, nt = 0, mode = kDual;
  bool walk = false, grouped = false, ship = false;
  size_t tile_kib = 128, pg = 0, rot = 0;
};

using LaunchFn = void (*)(const SegArr&, const Shape&, v4*, hipStream_t);

template <int BS, bool WALK, int U, bool G, int NT, int MODE>
void Launch(const SegArr& da, const Shape& sh, v4* sink, hipStream_t s) {
  size_t total = da.prefix[da.n];
  size_t cpb = sh.tile_kib * 1024 / 16;
  size_t ntiles = (total + cpb - 1) / cpb;
  size_t grid = sh.pg ? std::min(ntiles, 256 * sh.pg) : ntiles;
  hipLaunchKernelGGL((dw_kernel<BS, WALK, U, G, NT, MODE>), dim3(static_cast<unsigned>(grid)),
                     dim3(BS), 0, s, da, cpb, ntiles, sh.rot, sink);
}

template <int BS, int U, bool G>
LaunchFn PickNt(int nt) {
  switch (nt) {
    case 0: return Launch<BS, false, U, G, 0, kDual>;
    case 1: return Launch<BS, false, U, G, 1, kDual>;
    case 2: return Launch<BS, false, U, G, 2, kDual>;
    case 3: return Launch<BS, false, U, G, 3, kDual>;
  }
  return nullptr;
}
template <int BS>
LaunchFn PickU(int u, bool g, int nt) {
  switch (u) {
    case 1: return PickNt<BS, 1, false>(nt);
    case 2: return g ? PickNt<BS, 2, true>(nt) : PickNt<BS, 2, false>(nt);
    case 4: return g ? PickNt<BS, 4, true>(nt) : PickNt<BS, 4, false>(nt);
    case 8: return g ? PickNt<BS, 8, true>(nt) : PickNt<BS, 8, false>(nt);
  }
  return nullptr;
}
LaunchFn Pick(const Shape& sh) {
  if (sh.walk) return Launch<256, true, 1, false, 0, kDual>;
  if (sh.mode == kCopy) return Launch<256, false, 1, false, 0, kCopy>;
  if (sh.mode == kFill) return Launch<256, false, 1, false, 0, kFill>;
  if (sh.mode == kRead) return Launch<256, false, 1, false, 0, kRead>;
  switch (sh.bs) {
    case 256: return PickU<256>(sh.u, sh.grouped, sh.nt);
    case 512: return PickU<512>(sh.u, sh.grouped, sh.nt);
    case 1024: return PickU<1024>(sh.u, sh.grouped, sh.nt);
  }
  return nullptr;
}

bool ParseShape(const std::string& name, Shape* sh) {
  size_t at = 0;
  bool first = true;
  while (at <= name.size()) {
    size_t colon = name.find(':', at);
    if (colon == std::string::npos) colon = name.size();
    std::string tok = name.substr(at, colon - at);
    at = colon + 1;
    auto num = [&tok](size_t skip) { return strtoull(tok.c_str() + skip, nullptr, 10); };
    if (first) {
      first = false;
      if (tok == "ship") {
        sh->ship = true;
      } else if (tok == "walk") {
        sh->walk = true;
      } else if (tok != "runs") {
        return false;
      }
    } else if (tok == "g") {
      sh->grouped = true;
    } else if (tok == "i") {
      sh->grouped = false;
    } else if (tok == "copy") {
      sh->mode = kCopy;
    } else if (tok == "fill") {
      sh->mode = kFill;
    } else if (tok == "read") {
      sh->mode = kRead;
    } else if (tok.compare(0, 2, "nt") == 0) {
      sh->nt = static_cast<int>(num(2));
    } else if (tok.compare(0, 2, "pg") == 0) {
      sh->pg = num(2);
    } else if (tok.compare(0, 2, "bs") == 0) {
      sh->bs = static_cast<int>(num(2));
    } else if (tok.compare(0, 3, "rot") == 0) {
      sh->rot = num(3);
    } else if (tok[0] == 'u') {
      sh->u = static_cast<int>(num(1));
    } else if (tok[0] == 't') {
      sh->tile_kib = num(1);
    } else {
      return false;
    }
  }
  if (sh->tile_kib == 0 || sh->nt < 0 || sh->nt > 3) return false;
  return sh->ship || Pick(*sh) != nullptr;
}

const char* kDefaultVariants =
    // reference rows first
    "ship,runs:copy,runs:fill,runs:read,"
    // the restructuring
    "walk,runs,"
    // loads in flight, stores grouped / interleaved
    "runs:u2:g,runs:u2:i,runs:u4:g,runs:u4:i,runs:u8:g,runs:u8:i,"
    // resident waves per CU: 256*k blocks of 4 waves on 256 CUs
    "runs:pg2,runs:pg4,runs:pg8,"
    // nontemporal hints
    "runs:nt1,runs:nt2,runs:nt3,"
    // tile geometry (124 KiB = 31 * 4 KiB), rotated start (13 KiB * tile)
    "runs:t8,runs:t32,runs:t512,runs:t124,runs:rot832,"
    // block size
    "runs:bs512,runs:bs1024";

__global__ void pattern_kernel(v4* p, size_t n, unsigned salt) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n; i += stride) {
    unsigned x = static_cast<unsigned>(i) * 2654435761u + salt;
    v4 v = {x, x ^ 0x9e3779b9u, x * 31u + 7u, ~x};
    p[i] = v;
  }
}

__global__ void mismatch_kernel(const v4* a, const v4* b, size_t n, unsigned long long* bad) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  unsigned long long local = 0;
  for (; i < n; i += stride) {
    v4 x = a[i], y = b[i];
    if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) ++local;
  }
  if (local) atomicAdd(bad, local);
}

struct Variant {
  std::string name;
  Shape shape;
  LaunchFn fn = nullptr;
  std::vector<float> us;         // every timed launch
  std::vector<float> us_set[2];  // the same, split by buffer set
};

}  // namespace

int main(int argc, char** argv) {
  int rounds = 30, nseg = 16;
  size_t seg_mb = 64;
  std::string variants = kDefaultVariants;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--rounds" && i + 1 < argc) {
      rounds = atoi(argv[++i]);
    } else if (a == "--variants" && i + 1 < argc) {
      variants = argv[++i];
    } else if (a == "--segments" && i + 1 < argc) {
      nseg = atoi(argv[++i]);
    } else if (a == "--seg-mb" && i + 1 < argc) {
      seg_mb = strtoull(argv[++i], nullptr, 10);
    } else if (a == "--list") {
      printf("%s\n", kDefaultVariants);
      return 0;
    } else {
      fprintf(stderr, "usage: %s [--rounds N] [--variants a,b,...] [--segments N] [--seg-mb N] [--list]\n",
              argv[0]);
      return 2;
    }
  }
  if (rounds < 1 || nseg < 1 || nseg > kMaxBatch || seg_mb < 1) {
    fprintf(stderr, "bad --rounds/--segments/--seg-mb\n");
    return 2;
  }
  std::vector<Variant> vs;
  for (size_t at = 0; at <= variants.size();) {
    size_t comma = variants.find(',', at);
    if (comma == std::string::npos) comma = variants.size();
    Variant v;
    v.name = variants.substr(at, comma - at);
    at = comma + 1;
    if (v.name.empty()) continue;
    if (!ParseShape(v.name, &v.shape)) {
      fprintf(stderr, "unknown variant '%s'\n", v.name.c_str());
      return 2;
    }
    if (!v.shape.ship) v.fn = Pick(v.shape);
    vs.push_back(v);
  }

  // two buffer sets used alternately; each holds nseg segments x 3 ranges,
  // far more than the 256 MiB Infinity Cache keeps between uses
  const size_t seg_bytes = seg_mb << 20, seg_chunks = seg_bytes / 16;
  const size_t slab = seg_bytes * nseg;
  char* base[2][3];
  SegArr sets[2];
  std::vector<Seg2> segs[2];
  for (int s = 0; s < 2; ++s) {
    for (int k = 0; k < 3; ++k) CHECK(hipMalloc(reinterpret_cast<void**>(&base[s][k]), slab));
    hipLaunchKernelGGL(pattern_kernel, dim3(8192), dim3(256), 0, nullptr,
                       reinterpret_cast<v4*>(base[s][2]), slab / 16, 17u + s);
    memset(&sets[s], 0, sizeof(SegArr));
    sets[s].n = nseg;
    for (int i = 0; i < nseg; ++i) {
      Seg2 sg{base[s][0] + i * seg_bytes, base[s][1] + i * seg_bytes, base[s][2] + i * seg_bytes,
              seg_bytes};
      sets[s].d[i] = sg;
      sets[s].prefix[i] = i * seg_chunks;
      segs[s].push_back(sg);
    }
    sets[s].prefix[nseg] = nseg * seg_chunks;
  }
  v4* sink;
  unsigned long long* bad;
  CHECK(hipMalloc(reinterpret_cast<void**>(&sink), 64));
  CHECK(hipMalloc(reinterpret_cast<void**>(&bad), 8));
  CHECK(hipDeviceSynchronize());

  auto run = [&](Variant& v, int set) {
    if (v.shape.ship) {
      xps::kern::BatchedAssign2(segs[set].data(), nseg, nullptr);
    } else {
      v.fn(sets[set], v.shape, sink, nullptr);
    }
  };

  // warm-up doubles as the check: both destinations of set 0 cleared, one
  // launch, compared chunk by chunk against the source
  for (auto& v : vs) {
    bool writes0 = v.shape.mode != kRead, writes1 = v.shape.mode == kDual || v.shape.mode == kFill;
    bool verify = v.shape.mode == kDual || v.shape.mode == kCopy;
    CHECK(hipMemsetAsync(base[0][0], 0, slab, nullptr));
    CHECK(hipMemsetAsync(base[0][1], 0, slab, nullptr));
    CHECK(hipMemsetAsync(bad, 0, 8, nullptr));
    run(v, 0);
    CHECK(hipGetLastError());
    if (verify) {
      for (int k = 0; k < 2; ++k) {
        if ((k == 0 && !writes0) || (k == 1 && !writes1)) continue;
        hipLaunchKernelGGL(mismatch_kernel, dim3(8192), dim3(256), 0, nullptr,
                           reinterpret_cast<const v4*>(base[0][k]),
                           reinterpret_cast<const v4*>(base[0][2]), slab / 16, bad);
      }
      unsigned long long h = 0;
      CHECK(hipMemcpy(&h, bad, 8, hipMemcpyDeviceToHost));
      if (h) {
        fprintf(stderr, "variant %s: %llu chunks differ from the source\n", v.name.c_str(), h);
        return 1;
      }
    }
    run(v, 1);
    CHECK(hipDeviceSynchronize());
  }

  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (int r = 0; r < rounds; ++r) {
    for (size_t k = 0; k < vs.size(); ++k) {
      Variant& v = vs[k];
      int set = static_cast<int>((r + k) & 1);
      CHECK(hipEventRecord(e0, nullptr));
      run(v, set);
      CHECK(hipEventRecord(e1, nullptr));
      CHECK(hipEventSynchronize(e1));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      v.us.push_back(ms * 1000.f);
      v.us_set[set].push_back(ms * 1000.f);
    }
  }

  printf("# %d segments x %zu MiB, %d rounds, us per segment (launch time / %d)\n", nseg, seg_mb,
         rounds, nseg);
  printf("%-28s %9s %9s %9s %8s %9s %9s\n", "variant", "median", "min", "max", "TB/s", "med set0",
         "med set1");
  for (auto& v : vs) {
    std::sort(v.us.begin(), v.us.end());
    double med = v.us[v.us.size() / 2] / nseg, mn = v.us.front() / nseg, mx = v.us.back() / nseg;
    int streams = v.shape.mode == kDual ? 3 : v.shape.mode == kRead ? 1 : 2;
    double tbs = static_cast<double>(seg_bytes) * streams / (med * 1e-6) / 1e12;
    double ms[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
      std::sort(v.us_set[k].begin(), v.us_set[k].end());
      if (!v.us_set[k].empty()) ms[k] = v.us_set[k][v.us_set[k].size() / 2] / nseg;
    }
    printf("%-28s %9.2f %9.2f %9.2f %8.3f %9.2f %9.2f\n", v.name.c_str(), med, mn, mx, tbs, ms[0],
           ms[1]);
  }
  return 0;
}
