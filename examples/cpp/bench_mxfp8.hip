// One-process timing of the MXFP8 kernels (csrc/mxfp8.hip) against the
// copy kernel at equal traffic. Links kernels.hip and mxfp8.hip only: no
// cluster, no Python.
//
//   build/bench_mxfp8 [--rounds N]
//
// Cases: one key of 1, 4 and 64 MiB of fp32, and the ResNet-50 gradient
// bucket list (4 MiB partitions, ps_lite_amd/models/resnet50_buckets.py)
// in one call. Per case it times
//   quantize      fp32 -> packed            (reads 4 B, writes 1.03 B per element)
//   quantize-b    the same, batched
//   dequantize    packed -> fp32            (reads 1.03, writes 4)
//   dequantize-b  the same, batched
//   accumulate    acc += D(packed)          (reads 5.03, writes 4)
//   finish        out = Q(acc + D(packed))  (reads 5.03, writes 1.03)
// and kern::DenseAssign moving the same read + write byte total, every
// launch between its own pair of HIP events, over 6 or more buffer sets
// (1.5 GiB or more) in rotation, so that a timed launch finds nothing of its
// buffers in the 256 MiB Infinity Cache. Accumulate, finish and the -b rows
// take the bucket list as one batched call (one launch per 64 segments);
// the quantize and dequantize rows run the single kernels once per bucket,
// timed as one sequence, for comparison. Before timing, the batched
// quantize and dequantize of set 0 are compared byte for byte with the
// single kernels' output, every segment. Output: GB/s of each kernel's own
// traffic and its ratio to the copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../csrc/kernels.h"
#include "../../csrc/mxfp8.h"

#define CHECK(x)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

namespace {

using xps::kern::MxSeg;
using xps::kern::MxWorkSeg;
namespace mx = xps::mx;

// finite values with block maxima spread over ~2^16, some exact zeros
__global__ void pattern_kernel(float* p, size_t n, unsigned salt) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n; i += stride) {
    unsigned x = (static_cast<unsigned>(i) + salt) * 2654435761u;
    x ^= x >> 15;
    float unit = static_cast<float>(static_cast<int>(x & 0xffffu) - 32768) / 32768.0f;
    float mag = ldexpf(1.0f, static_cast<int>((i / 32) % 17) - 8);
    p[i] = (x >> 28) == 0 ? 0.0f : unit * mag;
  }
}

std::vector<size_t> Rn50BucketElems() {
  std::vector<size_t> sizes;
  auto conv = [&sizes](size_t out_c, size_t in_c, size_t k) {
    sizes.push_back(out_c * in_c * k * k);
  };
  auto bn = [&sizes](size_t c) {
    sizes.push_back(c);
    sizes.push_back(c);
  };
  conv(64, 3, 7);
  bn(64);
  const size_t stages[4][3] = {{64, 3, 64}, {128, 4, 256}, {256, 6, 512}, {512, 3, 1024}};
  for (auto& st : stages) {
    size_t planes = st[0];
    for (size_t b = 0; b < st[1]; ++b) {
      size_t inp = b == 0 ? st[2] : planes * 4;
      conv(planes, inp, 1);
      bn(planes);
      conv(planes, planes, 3);
      bn(planes);
      conv(planes * 4, planes, 1);
      bn(planes * 4);
      if (b == 0) {
        conv(planes * 4, inp, 1);
        bn(planes * 4);
      }
    }
  }
  sizes.push_back(1000 * 2048);
  sizes.push_back(1000);
  std::vector<size_t> buckets;
  const size_t part = (4u << 20) / 4;
  for (size_t n : sizes) {
    for (; n > part; n -= part) buckets.push_back(part);
    if (n) buckets.push_back(n);
  }
  return buckets;
}

// one rotation slot: every segment's fp32 source, packed form, accumulator
// and packed output, carved from four slabs
struct BufSet {
  float* f32;
  float* acc;
  char* packed;
  char* out;
  std::vector<MxSeg> segs;     // acc, packed, out per segment
  std::vector<float*> src;     // fp32 source per segment
  std::vector<float*> dq_dst;  // dequantize target per segment (the acc slab)
  std::vector<MxWorkSeg> qsegs;   // batched quantize: src -> out
  std::vector<MxWorkSeg> dqsegs;  // batched dequantize: packed -> dq_dst
};

struct Case {
  std::string name;
  std::vector<size_t> elems;  // per segment
};

double Median(std::vector<float>* v) {
  std::sort(v->begin(), v->end());
  return (*v)[v->size() / 2];
}

}  // namespace

int main(int argc, char** argv) {
  int rounds = 20;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--rounds") && i + 1 < argc) {
      rounds = atoi(argv[++i]);
    } else {
      fprintf(stderr, "usage: %s [--rounds N]\n", argv[0]);
      return 2;
    }
  }
  if (rounds < 1) return 2;

  std::vector<Case> cases = {{"1 MiB key", {(1u << 20) / 4}},
                             {"4 MiB key", {(4u << 20) / 4}},
                             {"64 MiB key", {(64u << 20) / 4}},
                             {"rn50 buckets", Rn50BucketElems()}};
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  printf("# %d rounds per kernel, median launch time; GB/s = the kernel's own read + write bytes\n",
         rounds);
  printf("%-14s %-12s %10s %10s %10s %8s\n", "case", "kernel", "us", "GB/s", "copy GB/s", "ratio");

  for (const Case& c : cases) {
    size_t f32_bytes = 0, packed_bytes = 0;
    std::vector<size_t> f32_off, packed_off;
    for (size_t n : c.elems) {
      f32_off.push_back(f32_bytes);
      packed_off.push_back(packed_bytes);
      // fp32 ranges sized in whole superblocks: the accumulator needs them
      f32_bytes += mx::MxSuperblocks(n) * mx::kSuperF32Bytes;
      packed_bytes += mx::MxPackedBytes(n);
    }
    // the two fp32 slabs carry a quarter of slack: the copy that matches
    // accumulate's traffic moves 4.5 bytes per element each way
    size_t slab_bytes = (f32_bytes / 4 * 5 + 15) & ~size_t{15};
    size_t footprint = 2 * slab_bytes + 2 * packed_bytes;
    // A round times the kernel on set `at` and the copy on set `at + nsets/2`,
    // and leaves both warm. With 6 sets or more neither is the next round's
    // kernel or copy set: a set comes up again three rounds later at the
    // soonest, after the other sets' traffic (1.5 GiB of sets in all, against
    // 256 MiB of Infinity Cache) has gone through.
    size_t nsets = std::max<size_t>(6, ((1536u << 20) + footprint - 1) / footprint);
    nsets = std::min<size_t>(nsets, 640);
    std::vector<BufSet> sets(nsets);
    for (size_t s = 0; s < nsets; ++s) {
      BufSet& b = sets[s];
      CHECK(hipMalloc(reinterpret_cast<void**>(&b.f32), slab_bytes));
      CHECK(hipMalloc(reinterpret_cast<void**>(&b.acc), slab_bytes));
      CHECK(hipMalloc(reinterpret_cast<void**>(&b.packed), packed_bytes));
      CHECK(hipMalloc(reinterpret_cast<void**>(&b.out), packed_bytes));
      hipLaunchKernelGGL(pattern_kernel, dim3(4096), dim3(256), 0, nullptr, b.f32, slab_bytes / 4,
                         static_cast<unsigned>(17 + s));
      for (size_t i = 0; i < c.elems.size(); ++i) {
        float* src = b.f32 + f32_off[i] / 4;
        float* acc = b.acc + f32_off[i] / 4;
        b.src.push_back(src);
        b.dq_dst.push_back(acc);
        b.segs.push_back(MxSeg{acc, b.packed + packed_off[i], b.out + packed_off[i],
                               mx::MxPackedBytes(c.elems[i])});
        b.qsegs.push_back(MxWorkSeg{src, b.out + packed_off[i], c.elems[i]});
        b.dqsegs.push_back(MxWorkSeg{acc, b.packed + packed_off[i], c.elems[i]});
        xps::kern::MxQuantize(src, c.elems[i], b.packed + packed_off[i], nullptr);
      }
      int nseg = static_cast<int>(b.segs.size());
      xps::kern::BatchedMxAccumulate(b.segs.data(), nseg, /*assign=*/true, nullptr);
    }
    CHECK(hipDeviceSynchronize());

    // check set 0 against the host reference before timing anything
    {
      size_t n = c.elems[0];
      std::vector<float> h(n), back(n), want(n);
      std::vector<uint8_t> p(mx::MxPackedBytes(n)), hp(mx::MxPackedBytes(n));
      CHECK(hipMemcpy(h.data(), sets[0].src[0], n * 4, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(p.data(), sets[0].packed, p.size(), hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(back.data(), sets[0].acc, n * 4, hipMemcpyDeviceToHost));
      mx::MxQuantizeHost(h.data(), n, hp.data());
      mx::MxDequantizeHost(hp.data(), n, want.data());
      size_t bad = 0;
      for (size_t i = 0; i < n; ++i) bad += back[i] != want[i];
      for (size_t sb = 0; sb < mx::MxSuperblocks(n); ++sb) {
        bad += memcmp(&p[sb * mx::kSuperBytes], &hp[sb * mx::kSuperBytes], mx::kSuperScales) != 0;
      }
      if (bad) {
        fprintf(stderr, "%s: %zu mismatches against the host reference\n", c.name.c_str(), bad);
        return 1;
      }
    }

    // the batched worker-side pair against the single kernels on set 0:
    // every byte of every segment's packed form, then of the fp32 slab
    // (0xFF-filled first, so floats past a segment's n count too)
    {
      BufSet& b = sets[0];
      int nseg = static_cast<int>(b.segs.size());
      std::vector<uint8_t> one(packed_bytes), many(packed_bytes);
      CHECK(hipMemset(b.out, 0xFF, packed_bytes));
      xps::kern::BatchedMxQuantize(b.qsegs.data(), nseg, nullptr);
      CHECK(hipMemcpy(one.data(), b.packed, packed_bytes, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(many.data(), b.out, packed_bytes, hipMemcpyDeviceToHost));
      size_t bad = 0;
      for (size_t i = 0; i < packed_bytes; ++i) bad += one[i] != many[i];
      if (bad) {
        fprintf(stderr, "%s: batched quantize differs from the single kernel in %zu bytes\n",
                c.name.c_str(), bad);
        return 1;
      }
      std::vector<uint8_t> fone(f32_bytes), fmany(f32_bytes);
      CHECK(hipMemset(b.acc, 0xFF, f32_bytes));
      for (int i = 0; i < nseg; ++i) {
        xps::kern::MxDequantize(b.segs[i].in, c.elems[i], b.dq_dst[i], 1.0f, nullptr);
      }
      CHECK(hipMemcpy(fone.data(), b.acc, f32_bytes, hipMemcpyDeviceToHost));
      CHECK(hipMemset(b.acc, 0xFF, f32_bytes));
      xps::kern::BatchedMxDequantize(b.dqsegs.data(), nseg, 1.0f, nullptr);
      CHECK(hipMemcpy(fmany.data(), b.acc, f32_bytes, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < f32_bytes; ++i) bad += fone[i] != fmany[i];
      if (bad) {
        fprintf(stderr, "%s: batched dequantize differs from the single kernel in %zu bytes\n",
                c.name.c_str(), bad);
        return 1;
      }
      xps::kern::BatchedMxAccumulate(b.segs.data(), nseg, /*assign=*/true, nullptr);
      CHECK(hipDeviceSynchronize());
    }

    double n_total = 0;
    for (size_t n : c.elems) {
      n_total += static_cast<double>(mx::MxSuperblocks(n) * mx::kSuperElems);
    }
    const double pk = 528.0 / 512.0;
    struct Kern {
      const char* name;
      double bytes;  // read + write
      int id;
    } kerns[6] = {{"quantize", n_total * (4 + pk), 0},
                  {"quantize-b", n_total * (4 + pk), 4},
                  {"dequantize", n_total * (4 + pk), 1},
                  {"dequantize-b", n_total * (4 + pk), 5},
                  {"accumulate", n_total * (8 + pk), 2},
                  {"finish", n_total * (4 + 2 * pk), 3}};
    for (const Kern& k : kerns) {
      // the copy moves half of the kernel's traffic in and half out
      size_t copy_bytes = static_cast<size_t>(k.bytes / 2) & ~size_t{15};
      copy_bytes = std::min(copy_bytes, slab_bytes);
      std::vector<float> us, us_copy;
      for (int r = -2; r < rounds; ++r) {
        size_t at = static_cast<size_t>(r + 2) % nsets;
        BufSet& b = sets[at];
        int nseg = static_cast<int>(b.segs.size());
        CHECK(hipEventRecord(e0, nullptr));
        switch (k.id) {
          case 0:
            for (int i = 0; i < nseg; ++i) {
              xps::kern::MxQuantize(b.src[i], c.elems[i], b.segs[i].out, nullptr);
            }
            break;
          case 1:
            for (int i = 0; i < nseg; ++i) {
              xps::kern::MxDequantize(b.segs[i].in, c.elems[i], b.dq_dst[i], 1.0f, nullptr);
            }
            break;
          case 2:
            xps::kern::BatchedMxAccumulate(b.segs.data(), nseg, /*assign=*/false, nullptr);
            break;
          case 4:
            xps::kern::BatchedMxQuantize(b.qsegs.data(), nseg, nullptr);
            break;
          case 5:
            xps::kern::BatchedMxDequantize(b.dqsegs.data(), nseg, 1.0f, nullptr);
            break;
          default:
            xps::kern::BatchedMxFinish(b.segs.data(), nseg, nullptr);
        }
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) us.push_back(ms * 1000.f);
        // accumulate ran: put the accumulator back (untimed) so values stay finite
        if (k.id == 2) xps::kern::BatchedMxAccumulate(b.segs.data(), nseg, true, nullptr);

        BufSet& cb = sets[(at + nsets / 2) % nsets];  // nsets >= 6: cold, and not used next
        CHECK(hipEventRecord(e0, nullptr));
        xps::kern::DenseAssign(cb.acc, cb.f32, copy_bytes, nullptr);
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) us_copy.push_back(ms * 1000.f);
        // the copy overwrote the accumulator slab: rebuild it (untimed)
        xps::kern::BatchedMxAccumulate(cb.segs.data(), static_cast<int>(cb.segs.size()), true,
                                       nullptr);
      }
      CHECK(hipGetLastError());
      double med = Median(&us), med_copy = Median(&us_copy);
      double gbs = k.bytes / (med * 1e-6) / 1e9;
      double gbs_copy = 2.0 * copy_bytes / (med_copy * 1e-6) / 1e9;
      printf("%-14s %-12s %10.2f %10.1f %10.1f %8.2f\n", c.name.c_str(), k.name, med, gbs, gbs_copy,
             gbs / gbs_copy);
      fflush(stdout);
    }
    for (BufSet& b : sets) {
      CHECK(hipFree(b.f32));
      CHECK(hipFree(b.acc));
      CHECK(hipFree(b.packed));
      CHECK(hipFree(b.out));
    }
  }
  return 0;
}
