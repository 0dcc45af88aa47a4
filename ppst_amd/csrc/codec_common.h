// What the image coders share across formats (png.hip, png_decode.hip, jpeg.hip, jpeg_decode.hip): the workgroup exclusive scan,
// the copy of a workspace slot to its place in a file, and the head of the decoders' workspaces with the kernel that fills it.
// What only the two PNG coders share is in png_common.h, what only the two JPEG coders share in jpeg_common.h.
#pragma once

// ------------------------------------------------------------------------------------------------------------------- scan
// Exclusive prefix of v over the NT threads of the workgroup, and the total; one barrier; `slot` alternates between consecutive
// calls.  The running base of a loop of scans stays with the caller, in the caller's own type (jpeg_layout_kernel's is unsigned
// and passes 2^31; the prefix within one call fits an int everywhere).
// The wave totals are joined in one of two ways; which one is faster depends on the caller (profiles/codec_common_ab.txt), so
// the caller chooses, and a change of the choice is to be measured:
//   SHFL = false  every thread reads the NT / 64 totals (broadcast LDS reads) and adds those of the waves in front of its own.
//                 The cheaper form where the scan sits in a hot loop of a workgroup with few waves (png_deflate_kernel).
//   SHFL = true   every wave scans the totals again in its first NT / 64 lanes with shuffles, and the lane number is opaque to
//                 the optimiser.  Needed in pd_inflate_kernel: written the plain way, the sixteen compares of the wave number
//                 against constants are made once per kernel and kept in scalar register pairs across the caller's loops,
//                 where they were spilled.
template <int NT, bool SHFL>
__device__ __forceinline__ int wg_scan(int v, int& total, int (*wave_tot)[NT / 64], int slot) {
  static_assert(NT % 64 == 0 && NT / 64 <= 64, "whole waves; one lane per wave total");
  int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (SHFL) asm volatile("" : "+v"(lane));
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_tot[slot][wave] = inc;
  __syncthreads();
  int before = 0;
  if (SHFL) {
    const int mine = wave_tot[slot][lane < NT / 64 ? lane : 0];
    int winc = lane < NT / 64 ? mine : 0;
#pragma unroll
    for (int o = 1; o < NT / 64; o <<= 1) {
      const int t = __shfl_up(winc, o, 64);
      if (lane >= o) winc += t;
    }
    total = __shfl(winc, NT / 64 - 1, 64);
    before = __shfl(winc - mine, wave, 64);
  } else {
    int all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
      const int t = wave_tot[slot][w];
      before += w < wave ? t : 0;
      all += t;
    }
    total = all;
  }
  return before + inc - v;
}

// ------------------------------------------------------------------------------------------------------------ slot -> file
// The whole workgroup (NT threads) copies n bytes from a 16-byte-aligned slot to any byte alignment in the file: the bytes up to
// the file's first aligned word, aligned words, the tail bytes.
template <int NT>
__device__ __forceinline__ void slot_to_file(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, unsigned n) {
  const unsigned lead = (unsigned)((4 - ((uintptr_t)dst & 3)) & 3);
  if (threadIdx.x < lead && threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x];
  if (n <= lead) return;
  const unsigned words = (n - lead) >> 2;
  for (unsigned i = threadIdx.x; i < words; i += NT) {
    const unsigned char* q = src + lead + 4 * i;
    *reinterpret_cast<unsigned*>(dst + lead + 4 * i) = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
  }
  const unsigned done = lead + 4 * words;
  if (threadIdx.x < n - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

// ------------------------------------------------------------------------------------------- the decoders' workspace head
// int32 rounds[B], then Img plan[B] (each rounded up to 16 bytes), then every image's arrays.  Img is the format's own struct:
// geometry g, layout l (l.total: bytes of the image's arrays) and base_off, where those arrays start.  The format's part of the
// plan is an overload of codec_fill(descriptor, subseq_words, Img*): geometry and layout from one descriptor.
__host__ __device__ inline int64_t a16(int64_t v) { return (v + 15) & ~(int64_t)15; }

template <class Img>
__host__ __device__ inline int64_t head_bytes(int B) { return a16((int64_t)B * 4) + a16((int64_t)B * (int64_t)sizeof(Img)); }

// the plan of image i (uniform loads of the fields a kernel uses: geometry and layout are worked out once per call, not per thread)
template <class Img>
__device__ __forceinline__ const Img& open_plan(int B, void* work, int i) {
  return ((const Img*)((unsigned char*)work + a16((int64_t)B * 4)))[i];
}

// one workgroup: every image's plan (a serial prefix over the B images places them), status and round counts to zero
template <class Img, class Desc>
__global__ __launch_bounds__(256) void plan_kernel(const Desc* __restrict__ descs, int B, int sw, void* work, int* __restrict__ status) {
  int* rounds = (int*)work;
  Img* plans = (Img*)((unsigned char*)work + a16((int64_t)B * 4));
  for (int i = threadIdx.x; i < B; i += 256) {
    rounds[i] = 0; status[i] = 0;
    codec_fill(descs[i], sw, &plans[i]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t at = head_bytes<Img>(B);
    for (int i = 0; i < B; ++i) {
      plans[i].base_off = at;
      at += plans[i].l.total;
    }
  }
}
