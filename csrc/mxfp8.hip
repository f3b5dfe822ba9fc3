// CDNA4 (gfx950) kernels of the MXFP8 wire format (mxfp8.h): quantize and
// dequantize on the worker side, accumulate and finish on the server side.
//
// Streaming kernels under the rules of kernels.hip: 16 B per lane per
// instruction, 64-wide wavefronts.
// Where codes are produced (quantize, finish) one lane owns 16 consecutive
// elements (four float4 of fp32, one uint4 of codes), two adjacent lanes
// make a 32-element block and share its amax through one cross-lane
// exchange, 32 lanes make a superblock and a wavefront makes two. The 16
// scale bytes of a superblock are collected into four dwords and stored by
// its first four lanes.
// Where fp32 is produced (dequantize, accumulate) no lane needs its
// neighbour, and one lane owns 4 consecutive elements per step instead: one
// dword of codes in, one float4 out, so that a wavefront's store covers
// 1 KiB without gaps, four such steps in flight per lane. Rates against the
// copy kernel are in profiles/mxfp8_kernels.md.
//
// fp32 <-> e4m3 goes through v_cvt_pk_fp8_f32 / v_cvt_pk_f32_fp8 (OCP
// e4m3fn on this target). Values are clamped to +-448 first, so the
// instruction's overflow mode never matters.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "kernels.h"
#include "mxfp8.h"
#include "tile_runs.h"

namespace xps {
namespace kern {

namespace {

constexpr int kLaneElems = 16;                    // elements owned by one lane
constexpr int kSuperLanes = 32;                   // lanes per superblock
constexpr int kBlockSupers = kBlock / kSuperLanes;  // superblocks per block stride

typedef float float2v __attribute__((ext_vector_type(2)));

// kVec below: the fp32 pointer is 16 B-aligned and moves as float4; else
// element by element. A template argument, not a run-time flag: with both
// forms behind one branch the compiler merged them into dword accesses.
// 16 floats at p
template <bool kVec>
__device__ inline void Load16(const float* __restrict__ p, float (&v)[kLaneElems]) {
  if (kVec) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float4 t = p4[j];
      v[4 * j] = t.x;
      v[4 * j + 1] = t.y;
      v[4 * j + 2] = t.z;
      v[4 * j + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < kLaneElems; ++i) v[i] = p[i];
  }
}

// elements [base, base + 16) of src[0, n); those past n read as +0.0
template <bool kVec>
__device__ inline void Load16Bounded(const float* __restrict__ src, size_t base, size_t n,
                                     float (&v)[kLaneElems]) {
  if (base + kLaneElems <= n) {
    Load16<kVec>(src + base, v);
  } else {
#pragma unroll
    for (int i = 0; i < kLaneElems; ++i) v[i] = base + i < n ? src[base + i] : 0.0f;
  }
}

__device__ inline float Clamp448(float x) { return fminf(fmaxf(x, -448.0f), 448.0f); }

// Quantize this lane's half block: the block's amax is the larger of this
// lane's and its neighbour's (lane ^ 1). Returns the 16 codes; *byte is the
// block's scale byte (the same in both lanes of the pair).
__device__ inline uint4 Quant16(const float (&v)[kLaneElems], uint32_t* byte) {
  float amax = 0.0f;
#pragma unroll
  for (int i = 0; i < kLaneElems; ++i) amax = fmaxf(amax, fabsf(v[i]));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  uint32_t b = mx::ScaleByte(amax);
  float inv = mx::InvScale(b);
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(Clamp448(v[4 * j] * inv), Clamp448(v[4 * j + 1] * inv), r,
                                        false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(Clamp448(v[4 * j + 2] * inv),
                                        Clamp448(v[4 * j + 3] * inv), r, true);
    w[j] = static_cast<uint32_t>(r);
  }
  *byte = b;
  return uint4{w[0], w[1], w[2], w[3]};
}

// v = float(codes) * 2^(byte-127), exact. The scale is built from its bits,
// so byte 0 gives 0.0 where the host reference's ldexp gives 2^-127: equal
// inside the contract, where byte 0 heads all-zero blocks only, and
// different for other packed input.
__device__ inline void Dequant16(uint4 codes, uint32_t byte, float (&v)[kLaneElems]) {
  float scale = mx::BitsF32(byte << 23);
  uint32_t w[4] = {codes.x, codes.y, codes.z, codes.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w[j]), false);
    float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w[j]), true);
    v[4 * j] = lo.x * scale;
    v[4 * j + 1] = lo.y * scale;
    v[4 * j + 2] = hi.x * scale;
    v[4 * j + 3] = hi.y * scale;
  }
}

// unit u = 16 elements: superblock u / 32, lane slot u % 32 inside it
__device__ inline void LoadPacked(const uint8_t* __restrict__ packed, size_t u, uint4* codes,
                                  uint32_t* byte) {
  const uint8_t* sb = packed + (u / kSuperLanes) * mx::kSuperBytes;
  uint32_t slot = static_cast<uint32_t>(u % kSuperLanes);
  *codes = *reinterpret_cast<const uint4*>(sb + mx::kSuperScales + slot * 16);
  *byte = sb[slot >> 1];
}

constexpr int kQuadElems = 4;                                // elements per lane per step
constexpr int kSuperQuads = mx::kSuperElems / kQuadElems;  // 128 quads per superblock

// elements [4q, 4q + 4) of a packed stream as fp32, exact (scale byte 0
// reads as 0.0, see Dequant16)
__device__ inline float4 Dequant4(const uint8_t* __restrict__ packed, size_t q) {
  const uint8_t* sb = packed + (q / kSuperQuads) * mx::kSuperBytes;
  uint32_t slot = static_cast<uint32_t>(q % kSuperQuads);
  int w = *reinterpret_cast<const int*>(sb + mx::kSuperScales + slot * 4);
  float scale = mx::BitsF32(static_cast<uint32_t>(sb[slot >> 3]) << 23);
  float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  return float4{lo.x * scale, lo.y * scale, hi.x * scale, hi.y * scale};
}

template <bool kVec>
__device__ inline float4 Load4(const float* __restrict__ p) {
  if (kVec) return *reinterpret_cast<const float4*>(p);
  return float4{p[0], p[1], p[2], p[3]};
}

template <bool kVec>
__device__ inline void Store4(float* __restrict__ p, float4 v) {
  if (kVec) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
    p[3] = v.w;
  }
}

// Every lane of the superblock calls this together (the callers' loops
// keep or drop whole superblocks): the scale bytes are exchanged across
// its 32 lanes.
__device__ inline void StorePacked(uint8_t* __restrict__ packed, size_t u, uint4 codes,
                                   uint32_t byte) {
  uint8_t* sb = packed + (u / kSuperLanes) * mx::kSuperBytes;
  uint32_t slot = static_cast<uint32_t>(u % kSuperLanes);
  *reinterpret_cast<uint4*>(sb + mx::kSuperScales + slot * 16) = codes;
  // dword (slot & 3) holds blocks 4 * (slot & 3) + j, owned by lanes
  // 2 * block of this superblock's half of the wavefront
  int half = static_cast<int>(threadIdx.x & 63u) & kSuperLanes;
  int first = half + 8 * static_cast<int>(slot & 3u);
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    word |= static_cast<uint32_t>(__shfl(static_cast<int>(byte), first + 2 * j)) << (8 * j);
  }
  if (slot < 4) reinterpret_cast<uint32_t*>(sb)[slot] = word;
}

// packed = Q(src[0, n)) for the 16-element units u, u + stride, ... below
// end. Whole superblocks of lanes arrive together (StorePacked); a lane
// past n loads zeros.
template <bool kVec, class Stride>
__device__ __forceinline__ void QuantUnits(const float* src, size_t n, uint8_t* packed, size_t u,
                                           size_t end, Stride stride) {
  for (; u < end; u += stride) {
    float v[kLaneElems];
    Load16Bounded<kVec>(src, u * kLaneElems, n, v);
    uint32_t byte;
    uint4 codes = Quant16(v, &byte);
    StorePacked(packed, u, codes, byte);
  }
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    mx_quantize_kernel(const float* __restrict__ src, size_t n, uint8_t* __restrict__ packed,
                       size_t units) {
  size_t u = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  QuantUnits<kVec>(src, n, packed, u, units, stride);
}

constexpr int kQuadSteps = 4;  // independent quads in flight per lane

__device__ inline float4 Scale4(float4 v, float alpha) {
  return float4{v.x * alpha, v.y * alpha, v.z * alpha, v.w * alpha};
}

// dst[0, n) = D(packed) * alpha for the quads q, q + stride, ... below end:
// kQuadSteps quads per trip while they lie below whole_end <= n / 4, all of
// a lane's loads ahead of its stores, then quad by quad.
template <bool kVec, class Stride>
__device__ __forceinline__ void DequantQuads(const uint8_t* packed, size_t n, float* dst,
                                             float alpha, size_t q, size_t whole_end, size_t end,
                                             Stride stride) {
  for (; q + (kQuadSteps - 1) * stride < whole_end; q += kQuadSteps * stride) {
    float4 v[kQuadSteps];
#pragma unroll
    for (int j = 0; j < kQuadSteps; ++j) v[j] = Dequant4(packed, q + j * stride);
#pragma unroll
    for (int j = 0; j < kQuadSteps; ++j) {
      Store4<kVec>(dst + (q + j * stride) * kQuadElems, Scale4(v[j], alpha));
    }
  }
  for (; q < end; q += stride) {
    float4 v = Scale4(Dequant4(packed, q), alpha);
    size_t base = q * kQuadElems;
    if (base + kQuadElems <= n) {
      Store4<kVec>(dst + base, v);
    } else {  // the quad that holds element n - 1: nothing is written past n
      if (base < n) dst[base] = v.x;
      if (base + 1 < n) dst[base + 1] = v.y;
      if (base + 2 < n) dst[base + 2] = v.z;
    }
  }
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    mx_dequantize_kernel(const uint8_t* __restrict__ packed, size_t n, float* __restrict__ dst,
                         float alpha, size_t quads) {
  size_t q = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  DequantQuads<kVec>(packed, n, dst, alpha, q, n / kQuadElems, quads, stride);
}

// Server side, up to kMaxBatch segments concatenated in superblock space.
// Each block owns one contiguous tile of supers_per_block superblocks and
// takes it apart into runs (tile_runs.h, a chunk being one superblock), so
// the segment table is read with block-uniform values and the inner loop
// has uniform base pointers. No segment is empty.
// kOp: 0 = acc = D(in), 1 = acc += D(in), 2 = out = Q((acc or 0) + D(in))
// kVec: every segment's acc is 16 B-aligned
template <int kOp, bool kVec>
__global__ void __launch_bounds__(kBlock)
    batched_mx_kernel(SegTable<MxSeg> da, size_t supers_per_block) {
  TileRunIter it = TileRunsBegin(da.prefix, da.n, supers_per_block, blockIdx.x);
  TileRun run;
  while (TileRunsNext(da.prefix, &it, &run)) {
    float* __restrict__ acc = da.d[run.seg].acc;
    const uint8_t* __restrict__ in = static_cast<const uint8_t*>(da.d[run.seg].in);
    uint8_t* __restrict__ out = static_cast<uint8_t*>(da.d[run.seg].out);
    if (kOp != 2) {
      // fp32 out: 4 elements per lane per step, gapless stores
      size_t end = run.hi * kSuperQuads;
      size_t q = run.lo * kSuperQuads + threadIdx.x;
      // a whole tile is kQuadSteps strides of the block: all of a lane's
      // loads go out ahead of its stores
      for (; q + (kQuadSteps - 1) * kBlock < end; q += kQuadSteps * kBlock) {
        float4 v[kQuadSteps];
#pragma unroll
        for (int j = 0; j < kQuadSteps; ++j) v[j] = Dequant4(in, q + j * kBlock);
        if (kOp == 1) {
#pragma unroll
          for (int j = 0; j < kQuadSteps; ++j) {
            float4 a = Load4<kVec>(acc + (q + j * kBlock) * kQuadElems);
            v[j] = float4{a.x + v[j].x, a.y + v[j].y, a.z + v[j].z, a.w + v[j].w};
          }
        }
#pragma unroll
        for (int j = 0; j < kQuadSteps; ++j) {
          Store4<kVec>(acc + (q + j * kBlock) * kQuadElems, v[j]);
        }
      }
      for (; q < end; q += kBlock) {
        float4 v = Dequant4(in, q);
        float* p = acc + q * kQuadElems;
        if (kOp == 1) {
          float4 a = Load4<kVec>(p);
          v = float4{a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w};
        }
        Store4<kVec>(p, v);
      }
      continue;
    }
    // codes out: 16 elements per lane, whole superblocks of lanes
    size_t end = run.hi * kSuperLanes;
    for (size_t u = run.lo * kSuperLanes + threadIdx.x; u < end; u += kBlock) {
      uint4 codes;
      uint32_t byte;
      LoadPacked(in, u, &codes, &byte);
      float v[kLaneElems];
      Dequant16(codes, byte, v);
      if (acc != nullptr) {
        float a[kLaneElems];
        Load16<kVec>(acc + u * kLaneElems, a);
#pragma unroll
        for (int i = 0; i < kLaneElems; ++i) v[i] = a[i] + v[i];
      }
      uint32_t obyte;
      uint4 ocodes = Quant16(v, &obyte);
      StorePacked(out, u, ocodes, obyte);
    }
  }
}

void CheckPacked(const char* who, const void* packed, size_t nbytes) {
  if (!Aligned16(packed)) {
    throw std::invalid_argument(std::string(who) + ": packed pointer is not 16 B-aligned");
  }
  if (nbytes % mx::kSuperBytes) {
    throw std::invalid_argument(std::string(who) + ": packed length " + std::to_string(nbytes) +
                                " is not a multiple of 528");
  }
}

// kVec from a run-time test: launch(std::true_type or std::false_type)
template <class Launch>
void WithVec(bool vec, Launch launch) {
  if (vec) {
    launch(std::true_type{});
  } else {
    launch(std::false_type{});
  }
}

// a launch moves fp32 as float4 when every segment of its table can
template <class Seg>
bool TableAligned16(const SegTable<Seg>& da, float* Seg::*f32) {
  for (int i = 0; i < da.n; ++i) {
    if (!Aligned16(da.d[i].*f32)) return false;
  }
  return true;
}

// one stride of the block (8 superblocks, 16 KiB of fp32) per tile; a
// tile_cap grows the tile, in whole strides, until the grid fits it
size_t MxTile(size_t total, int tile_cap) {
  return TileChunks(total, kBlockSupers, kAnyBlocks, 0, tile_cap);
}

template <int kOp>
int LaunchBatchedMx(const char* who, const MxSeg* segs_host, int n, hipStream_t s, int tile_cap) {
  for (int i = 0; i < n; ++i) {
    CheckPacked(who, segs_host[i].in, segs_host[i].nbytes);
    if (kOp == 2) CheckPacked(who, segs_host[i].out, 0);
    if (kOp != 2 && segs_host[i].nbytes && !segs_host[i].acc) {
      throw std::invalid_argument(std::string(who) + ": null accumulator");
    }
  }
  return ForEachTable(
      segs_host, n, [](const MxSeg& sg) { return sg.nbytes / mx::kSuperBytes; },
      [&](const SegTable<MxSeg>& da, size_t total) {
        size_t spb = MxTile(total, tile_cap);
        WithVec(TableAligned16(da, &MxSeg::acc), [&](auto vec) {
          hipLaunchKernelGGL((batched_mx_kernel<kOp, decltype(vec)::value>),
                             dim3(TileGrid(total, spb)), dim3(kBlock), 0, s, da, spb);
        });
      });
}

// Worker side, up to kMaxBatch segments concatenated in superblock space
// and tiled like batched_mx_kernel: block-uniform table reads, uniform base
// pointers in the inner loops. A segment's last superblock may be partial
// (n is any positive count); no segment is empty.
// kVec: every segment's f32 is 16 B-aligned
template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    batched_mx_quantize_kernel(SegTable<MxWorkSeg> da, size_t supers_per_block) {
  TileRunIter it = TileRunsBegin(da.prefix, da.n, supers_per_block, blockIdx.x);
  TileRun run;
  while (TileRunsNext(da.prefix, &it, &run)) {
    QuantUnits<kVec>(da.d[run.seg].f32, da.d[run.seg].n,
                     static_cast<uint8_t*>(da.d[run.seg].packed),
                     run.lo * kSuperLanes + threadIdx.x, run.hi * kSuperLanes, kBlock);
  }
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    batched_mx_dequantize_kernel(SegTable<MxWorkSeg> da, float alpha, size_t supers_per_block) {
  TileRunIter it = TileRunsBegin(da.prefix, da.n, supers_per_block, blockIdx.x);
  TileRun run;
  while (TileRunsNext(da.prefix, &it, &run)) {
    size_t n = da.d[run.seg].n;
    // the run's quads end with the segment's elements, not with its last
    // superblock
    size_t run_end = run.hi * kSuperQuads;
    size_t quads = (n + kQuadElems - 1) / kQuadElems;
    size_t whole = n / kQuadElems;
    // a whole tile is kQuadSteps strides of the block
    DequantQuads<kVec>(static_cast<const uint8_t*>(da.d[run.seg].packed), n, da.d[run.seg].f32,
                       alpha, run.lo * kSuperQuads + threadIdx.x,
                       run_end < whole ? run_end : whole, run_end < quads ? run_end : quads,
                       kBlock);
  }
}

// kQuant: batched_mx_quantize_kernel, else batched_mx_dequantize_kernel
template <bool kQuant>
int LaunchBatchedMxWork(const char* who, const MxWorkSeg* segs_host, int n, float alpha,
                        hipStream_t s, int tile_cap) {
  for (int i = 0; i < n; ++i) {
    CheckPacked(who, segs_host[i].packed, 0);
    if (segs_host[i].n && !segs_host[i].f32) {
      throw std::invalid_argument(std::string(who) + ": null f32 pointer");
    }
  }
  return ForEachTable(
      segs_host, n, [](const MxWorkSeg& sg) { return mx::MxSuperblocks(sg.n); },
      [&](const SegTable<MxWorkSeg>& da, size_t total) {
        size_t spb = MxTile(total, tile_cap);
        dim3 grid(TileGrid(total, spb));
        WithVec(TableAligned16(da, &MxWorkSeg::f32), [&](auto vec) {
          constexpr bool kVec = decltype(vec)::value;
          if constexpr (kQuant) {
            hipLaunchKernelGGL(batched_mx_quantize_kernel<kVec>, grid, dim3(kBlock), 0, s, da, spb);
          } else {
            hipLaunchKernelGGL(batched_mx_dequantize_kernel<kVec>, grid, dim3(kBlock), 0, s, da,
                               alpha, spb);
          }
        });
      });
}

}  // namespace

void MxQuantize(const float* src, size_t n, void* packed, hipStream_t s, int grid_cap) {
  CheckPacked("MxQuantize", packed, 0);
  if (n == 0) return;
  size_t units = mx::MxSuperblocks(n) * kSuperLanes;
  dim3 grid(GridFor(units, 8192, grid_cap));
  uint8_t* out = static_cast<uint8_t*>(packed);
  WithVec(Aligned16(src), [&](auto vec) {
    hipLaunchKernelGGL(mx_quantize_kernel<decltype(vec)::value>, grid, dim3(kBlock), 0, s, src, n,
                       out, units);
  });
}

void MxDequantize(const void* packed, size_t n, float* dst, float alpha, hipStream_t s,
                  int grid_cap) {
  CheckPacked("MxDequantize", packed, 0);
  if (n == 0) return;
  size_t quads = (n + kQuadElems - 1) / kQuadElems;
  size_t lanes = (quads + kQuadSteps - 1) / kQuadSteps;
  dim3 grid(GridFor(lanes, 8192, grid_cap));
  const uint8_t* in = static_cast<const uint8_t*>(packed);
  WithVec(Aligned16(dst), [&](auto vec) {
    hipLaunchKernelGGL(mx_dequantize_kernel<decltype(vec)::value>, grid, dim3(kBlock), 0, s, in, n,
                       dst, alpha, quads);
  });
}

void MxAccumulate(float* acc, const void* packed, size_t nbytes, bool assign, hipStream_t s,
                  int grid_cap) {
  MxSeg sg{acc, packed, nullptr, nbytes};
  if (assign) {
    LaunchBatchedMx<0>("MxAccumulate", &sg, 1, s, grid_cap);
  } else {
    LaunchBatchedMx<1>("MxAccumulate", &sg, 1, s, grid_cap);
  }
}

void MxFinish(const float* acc_or_null, const void* packed_in, void* packed_out, size_t nbytes,
              hipStream_t s, int grid_cap) {
  MxSeg sg{const_cast<float*>(acc_or_null), packed_in, packed_out, nbytes};
  LaunchBatchedMx<2>("MxFinish", &sg, 1, s, grid_cap);
}

int BatchedMxAccumulate(const MxSeg* segs_host, int n, bool assign, hipStream_t s, int tile_cap) {
  return assign ? LaunchBatchedMx<0>("BatchedMxAccumulate", segs_host, n, s, tile_cap)
                : LaunchBatchedMx<1>("BatchedMxAccumulate", segs_host, n, s, tile_cap);
}

int BatchedMxFinish(const MxSeg* segs_host, int n, hipStream_t s, int tile_cap) {
  return LaunchBatchedMx<2>("BatchedMxFinish", segs_host, n, s, tile_cap);
}

int BatchedMxQuantize(const MxWorkSeg* segs_host, int n, hipStream_t s, int tile_cap) {
  return LaunchBatchedMxWork<true>("BatchedMxQuantize", segs_host, n, 1.0f, s, tile_cap);
}

int BatchedMxDequantize(const MxWorkSeg* segs_host, int n, float alpha, hipStream_t s,
                        int tile_cap) {
  return LaunchBatchedMxWork<false>("BatchedMxDequantize", segs_host, n, alpha, s, tile_cap);
}

}  // namespace kern
}  // namespace xps
