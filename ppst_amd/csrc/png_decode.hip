// PNG decode on the device: 8-bit grey / RGB / RGBA files of any origin -> uint8 HWC, equal to what Pillow reads (DESIGN.md "PNG
// decode on the device"; the format and the scheme: include/ppst_hip.h).  A batch holds files of different sizes and colour
// types: every kernel runs on a grid (largest per-image count, B) and a workgroup beyond its image's count leaves.
//   0. plan_kernel<PdImg>  one workgroup: every image's layout and place in the workspace, stored for the other kernels
//                          (codec_common.h, with the head of the workspace and the workgroup scan; the format's part: codec_fill)
//   1. pd_offsets_kernel   one workgroup per image: where every IDAT payload goes in the zlib stream (exclusive prefix over the
//                          chunk lengths), the zlib header, the image's counters to zero
//      pd_chunk_kernel     one workgroup per chunk: CRC-32 over type + data against the stored one; an IDAT payload is copied
//   2. pd_inflate_kernel   one workgroup per image: deflate blocks in order; per block the tables in LDS, the subsequence
//                          iteration to the fixed point in windows of one subsequence per lane, byte prefix, the write pass into
//                          raw / src
//   3. pd_jump_kernel      src[i] <- src[src[i]] in place, one launch per round; a round whose predecessor changed nothing leaves
//      pd_resolve_kernel   stream[i] = raw[src[i]], Adler-32 partial sums per 4096 bytes
//   4. pd_unfilter_kernel  one workgroup per image: Adler-32 against the trailer; the row filters undone, a row per lane, each
//                          lane one pixel behind the lane above it; HWC store
// Integer code throughout.  No workgroup waits for another: the stages meet at launch boundaries only, and inside a workgroup
// at barriers only.  Every loop over file data has a bound that does not depend on the data.
// Shared with the encoder (png_common.h): the CRC-32, the Paeth predictor, the code-length order, the joining of Adler-32 sums.
#include "common.h"
#include "codec_common.h"
#include "png_common.h"

#define PD_T 256                                // threads of the stream kernels
#define PD_CHUNK 4096                           // bytes of the stream per workgroup of pd_resolve_kernel: 16 per thread
#define PD_INF_T 1024                           // threads of the inflate and unfilter workgroups: subsequences per window
#define PD_SUBSEQ_DEFAULT 4                     // words: 128 bits (profiles/png_decode_time.txt)
#define PD_SUBSEQ_MAX 128                       // 4096 bits: a lane's byte count stays below 2^20 (258 bytes from 2 bits), a window's below 2^31
#define PD_ROUNDS_MAX 33                        // pointer-jumping launches: ceil(log2 n) + 1 <= 32
#define PD_DEAD 0xFFFFFFFFu                     // the exit of a subsequence that met the end of the block

__constant__ unsigned short PD_LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ unsigned char PD_LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ unsigned short PD_DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ unsigned char PD_DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

// ------------------------------------------------------------------------------------------------------------------ layout
struct PdGeom {
  int H, W, C, cout;
  int row;                  // 1 + W C
  int n;                    // H row: bytes of the inflated stream (< 2^31)
  unsigned L;               // bytes of the zlib stream (< 2^28)
  unsigned SB;              // bits per subsequence
  int nchunk;               // pieces of PD_CHUNK bytes of the stream
  int jumps;                // pointer-jumping rounds: ceil(log2 n) + 1
};
// byte offsets of one image's arrays from its base (each a multiple of 16)
struct PdLayout { int64_t soff, zs, raw, src, stream, part, cnt, total; };
// cnt: int32 [PD_ROUNDS_MAX] change counters, then [PD_ROUNDS_MAX] = the bit behind the final block

__host__ __device__ inline void pd_geom(const ppst_png_dec_image& d, int sw, PdGeom* g) {
  g->H = d.H; g->W = d.W; g->C = d.channels;
  g->cout = d.channels == 1 ? (d.expand_grey ? 3 : 1) : (d.channels == 4 && !d.drop_alpha ? 4 : 3);
  g->row = 1 + d.W * d.channels;
  g->n = d.H * g->row;
  g->L = (unsigned)d.idat_bytes;
  g->SB = 32u * (unsigned)(sw > 0 ? sw : PD_SUBSEQ_DEFAULT);
  g->nchunk = (int)(((int64_t)g->n + PD_CHUNK - 1) / PD_CHUNK);
  int lg = 0;
  while (lg < 31 && ((int64_t)1 << lg) < (int64_t)g->n) ++lg;
  g->jumps = lg + 1;
}

__host__ __device__ inline void pd_layout(const ppst_png_dec_image& d, const PdGeom& g, PdLayout* l) {
  int64_t at = 0;
  l->soff = at;   at = a16(at + ((int64_t)d.nidat + 1) * 4);
  l->zs = at;     at = a16(at + (int64_t)g.L + 16);
  l->raw = at;    at = a16(at + (int64_t)g.n);
  l->src = at;    at = a16(at + (int64_t)g.n * 4);
  l->stream = at; at = a16(at + (int64_t)g.n);
  l->part = at;   at = a16(at + (int64_t)g.nchunk * 8);
  l->cnt = at;    at = a16(at + (PD_ROUNDS_MAX + 1) * 4);
  l->total = at;
}

struct PdImg {                                  // what a workgroup needs of its image: written once by plan_kernel (codec_common.h)
  PdGeom g;
  PdLayout l;
  int64_t base_off;
};
__host__ __device__ inline void codec_fill(const ppst_png_dec_image& d, int sw, PdImg* im) {
  pd_geom(d, sw, &im->g);
  pd_layout(d, im->g, &im->l);
}

// a span as the kernels use it: clamped to the file, so that no field of the table can take a read outside the file's bytes
__device__ __forceinline__ bool pd_span(const ppst_png_dec_image& d, const ppst_png_span& s, unsigned* off, unsigned* len) {
  const bool ok = s.off >= 4 && s.len >= 0 && (int64_t)s.off + s.len <= d.file_len;
  *off = ok ? (unsigned)s.off : 4u;
  *len = ok ? (unsigned)s.len : 0u;
  return ok;
}

// ------------------------------------------------------------------------------------------------------------------- gather
__global__ __launch_bounds__(PD_T) void pd_offsets_kernel(const unsigned char* __restrict__ files, const ppst_png_dec_image* __restrict__ descs,
                                                          const ppst_png_span* __restrict__ spans, int B, void* work, int* __restrict__ status) {
  __shared__ int wt[2][PD_T / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  const PdImg& im = open_plan<PdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  const ppst_png_dec_image& d = descs[i];
  const ppst_png_span* sp = spans + d.span_off + d.first_idat;
  unsigned* soff = (unsigned*)(base + im.l.soff);
  int* cnt = (int*)(base + im.l.cnt);
  for (int k = tid; k < PD_ROUNDS_MAX + 1; k += PD_T) cnt[k] = 0;
  unsigned char* zs = base + im.l.zs;
  const int64_t zcap = a16((int64_t)im.g.L + 16);
  for (int64_t k = (int64_t)im.g.L + tid; k < zcap; k += PD_T) zs[k] = 0;        // the words behind the stream read as zero
  int run = 0, bad = 0;
  for (int c0 = 0; c0 < d.nidat; c0 += PD_T) {
    const int c = c0 + tid;
    unsigned off = 0, len = 0;
    if (c < d.nidat) bad |= !pd_span(d, sp[c], &off, &len);
    int tot;
    const int pre = wg_scan<PD_T, true>((int)len, tot, wt, 0);
    if (c < d.nidat) soff[c] = (unsigned)(run + pre);
    run += tot;
    __syncthreads();                                               // wt is reused by the next round
  }
  if (tid == 0) {
    soff[d.nidat] = (unsigned)run;
    if ((unsigned)run != im.g.L) bad = 1;
    // the zlib header: the first two bytes of the stream, wherever the chunk boundaries fall
    int have = 0, cmf = 0, flg = 0;
    for (int c = 0; c < d.nidat && have < 2; ++c) {
      unsigned off, len;
      pd_span(d, sp[c], &off, &len);
      for (unsigned k = 0; k < len && have < 2; ++k, ++have) (have ? flg : cmf) = files[d.file_off + off + k];
    }
    if (have < 2 || (cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 32) || ((cmf << 8) | flg) % 31 != 0) atomicOr(&status[i], PPST_PNG_S_ZLIB);
  }
  if (bad) atomicOr(&status[i], PPST_PNG_S_CRC);                     // (a span table the parser did not make)
}

__global__ __launch_bounds__(PD_T) void pd_chunk_kernel(const unsigned char* __restrict__ files, const ppst_png_dec_image* __restrict__ descs,
                                                        const ppst_png_span* __restrict__ spans, int B, void* work, int* __restrict__ status) {
  __shared__ unsigned crc;
  const int i = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  const ppst_png_dec_image& d = descs[i];
  if (j >= d.nspans) return;
  const PdImg& im = open_plan<PdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  const ppst_png_span& s = spans[d.span_off + j];
  unsigned off, len;
  if (!pd_span(d, s, &off, &len)) return;                            // (pd_offsets_kernel has set the status)
  if (tid == 0) crc = 0;
  __syncthreads();
  const unsigned char* p = files + d.file_off + off - 4;             // type + data
  const unsigned total = len + 4;
  const unsigned per = (total + PD_T - 1) / PD_T;
  const unsigned s0 = min(total, tid * per), s1 = min(total, s0 + per);
  if (s0 < s1) {
    unsigned c = s0 == 0 ? 0xFFFFFFFFu : 0u;
    for (unsigned k = s0; k < s1; ++k) c = crc_word(c, p[k], 1);
    atomicXor(&crc, crc_mul(crc_xpow8(total - s1), c));
  }
  __syncthreads();
  if (tid == 0 && (crc ^ 0xFFFFFFFFu) != s.crc) atomicOr(&status[i], PPST_PNG_S_CRC);
  const int q = j - d.first_idat;
  if (q >= 0 && q < d.nidat) {
    const unsigned* soff = (const unsigned*)(base + im.l.soff);
    const unsigned at = soff[q];
    unsigned char* zs = base + im.l.zs;
    for (unsigned k = tid; k < len; k += PD_T)
      if (at + k < im.g.L) zs[at + k] = p[4 + k];
  }
}

// ------------------------------------------------------------------------------------------------------------------ inflate
struct PdCode {                    // one canonical code: the first 9 bits in a table, longer codes by their length
  unsigned short lut[512];         // the next 9 bits of the stream -> (length << 9) | symbol, 0: no code of at most 9 bits
  unsigned short sorted[288];      // symbols by (length, symbol)
  int count[16];                   // codes per length
  unsigned first[16];              // the first code of a length (MSB first)
  int index[16];                   // where the length's symbols start in `sorted`
};
struct PdTabs {
  PdCode lit, dist;
  unsigned char lens[320];         // lit / len lengths, then the distance lengths
  unsigned short cl_lut[128];      // the code-length code: 7 bits -> (length << 8) | symbol
  unsigned short lbase[32], dbase[32];   // copies of the length / distance tables: a lookup per token, no address to keep
  unsigned char lext[32], dext[32];
  unsigned X[PD_INF_T];            // exits of the window's subsequences
  int wt[2][PD_INF_T / 64];
  int nl, nd;                      // symbols of the two alphabets of this block
  int btype, bfinal, stop;
  unsigned p;                      // bit position: the block's first token; behind the block once it has ended
  unsigned st_at, st_len;          // stored block: first byte, bytes
  int eob_lane;
  unsigned eob_p;
  int bits;                        // status bits collected by the workgroup
};

// 32 bits at bit p of the stream, LSB first (the array is zero for 16 bytes behind the stream: callers keep p below 8 L + 64)
__device__ __forceinline__ unsigned pd_peek(const unsigned* __restrict__ zw, unsigned p) {
  const unsigned w = p >> 5, sh = p & 31u;
  const unsigned lo = zw[w], hi = zw[w + 1];
  return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
}

// the symbol at the low end of v and its length; -1 (length 0): no such code
__device__ __forceinline__ int pd_sym(const PdCode& c, unsigned v, int& len) {
  const unsigned e = c.lut[v & 511u];
  if (e) { len = (int)(e >> 9); return (int)(e & 511u); }
  const unsigned rev = __brev(v);
  int hit_l = 0, hit_at = 0;                                        // (selects, no early exit: the lengths are few, the branches would nest)
#pragma unroll
  for (int l = 15; l >= 10; --l) {
    const unsigned code = rev >> (32 - l);
    const unsigned k = code - c.first[l];
    const bool hit = code >= c.first[l] && k < (unsigned)c.count[l];
    hit_l = hit ? l : hit_l;                                        // a prefix code: at most one length hits
    hit_at = hit ? c.index[l] + (int)k : hit_at;
  }
  len = hit_l;
  return hit_l ? (int)c.sorted[hit_at] : -1;
}

// count[], first[], index[] of a code from its lengths (one thread), zlib's verdict: 0 fine, 1 over-subscribed or incomplete
// (an incomplete code is let through when its longest length is 1, and a code of no symbols at all when `empty_ok`)
__device__ int pd_code_counts(PdCode& c, const unsigned char* lens, int n, bool empty_ok) {
  for (int l = 0; l < 16; ++l) c.count[l] = 0;
  for (int s = 0; s < n; ++s) c.count[lens[s] & 15]++;
  int left = 1, maxl = 0, idx = 0;
  unsigned code = 0;
  c.first[0] = 0; c.index[0] = 0;
  for (int l = 1; l <= 15; ++l) {
    code = (code + (unsigned)(l > 1 ? c.count[l - 1] : 0)) << 1;
    c.first[l] = code;
    c.index[l] = idx;
    idx += c.count[l];
    left = (left << 1) - c.count[l];
    if (left < 0) return 1;
    if (c.count[l]) maxl = l;
  }
  if (maxl == 0) return empty_ok ? 0 : 1;
  if (left > 0 && maxl != 1) return 1;
  return 0;
}

// every thread below n places its symbol: rank among the symbols of its length in front of it -> sorted[], the 9-bit table
__device__ __forceinline__ void pd_code_fill(PdCode& c, const unsigned char* lens, int n, int s) {
  if (s >= n) return;
  const int l = lens[s];
  if (!l) return;
  int rank = 0;
  for (int t = 0; t < s; ++t) rank += lens[t] == l;
  c.sorted[c.index[l] + rank] = (unsigned short)s;
  if (l <= 9) {
    const unsigned code = c.first[l] + (unsigned)rank;
    const unsigned rev = __brev(code) >> (32 - l);
    const unsigned short ent = (unsigned short)((l << 9) | s);
    for (unsigned f = 0; f < (1u << (9 - l)); ++f) c.lut[rev | (f << l)] = ent;
  }
}

// One token from bit p: kind 0 a literal (value in len), 1 a match (len, dist), 2 end of block, 3 a code no table defines (one bit
// on, or the bits of the part that was defined: both decodes walk alike).  A token takes at most 48 bits.
struct PdTok { unsigned p; int kind, len, dist; };
__device__ __forceinline__ PdTok pd_token(const PdTabs& T, const unsigned* __restrict__ zw, unsigned p) {
  PdTok o = {p, 3, 0, 0};
  unsigned v = pd_peek(zw, p);
  int l;
  const int sym = pd_sym(T.lit, v, l);
  if (sym < 0) { o.p = p + 1; return o; }
  p += (unsigned)l;
  o.p = p;
  if (sym < 256) { o.kind = 0; o.len = sym; return o; }
  if (sym == 256) { o.kind = 2; return o; }
  if (sym > 285) return o;
  const int eb = T.lext[sym - 257];
  o.len = T.lbase[sym - 257] + (int)((v >> l) & ((1u << eb) - 1u));
  p += (unsigned)eb;
  v = pd_peek(zw, p);
  const int ds = pd_sym(T.dist, v, l);
  if (ds < 0) { o.p = p + 1; return o; }
  p += (unsigned)l;
  o.p = p;
  if (ds > 29) return o;
  const int db = T.dext[ds];
  o.dist = T.dbase[ds] + (int)((v >> l) & ((1u << db) - 1u));
  o.p = p + (unsigned)db;
  o.kind = 1;
  return o;
}

// thread 0: the header of the block at T.p.  Leaves T.btype, T.bfinal, T.p (the first bit behind the header), for a stored block
// st_at / st_len, for a dynamic one lens[], nl, nd; T.stop and T.bits on a fault.
__device__ void pd_block_header(PdTabs& T, const unsigned* __restrict__ zw, const unsigned char* __restrict__ zs, unsigned L) {
  const unsigned nbits = L * 8u;
  unsigned p = T.p;
  if (p + 3 > nbits) { T.stop = 1; T.bits |= PPST_PNG_S_STREAM; return; }
  unsigned v = pd_peek(zw, p);
  T.bfinal = (int)(v & 1u);
  T.btype = (int)((v >> 1) & 3u);
  p += 3;
  if (T.btype == 3) { T.stop = 1; T.bits |= PPST_PNG_S_BTYPE; return; }
  if (T.btype == 0) {
    const unsigned at = (p + 7) >> 3;
    if (at + 4 > L) { T.stop = 1; T.bits |= PPST_PNG_S_STORED; return; }
    const unsigned len = zs[at] | ((unsigned)zs[at + 1] << 8), nlen = zs[at + 2] | ((unsigned)zs[at + 3] << 8);
    if ((len ^ 0xFFFFu) != nlen || at + 4 + len > L) { T.stop = 1; T.bits |= PPST_PNG_S_STORED; return; }
    T.st_at = at + 4; T.st_len = len;
    T.p = (at + 4 + len) * 8u;
    return;
  }
  if (T.btype == 1) { T.nl = 288; T.nd = 32; T.p = p; return; }   // (the lengths are filled by all threads)
  if (p + 14 > nbits) { T.stop = 1; T.bits |= PPST_PNG_S_STREAM; return; }
  v = pd_peek(zw, p);
  const int hlit = (int)(v & 31u) + 257, hdist = (int)((v >> 5) & 31u) + 1, hclen = (int)((v >> 10) & 15u) + 4;
  p += 14;
  if (hlit > 286 || hdist > 30) { T.stop = 1; T.bits |= PPST_PNG_S_LENGTHS; return; }
  if (p + 3u * (unsigned)hclen > nbits) { T.stop = 1; T.bits |= PPST_PNG_S_STREAM; return; }
  // the code-length code: its 19 lengths live in lens[300 .. 318] while its table is built
  unsigned char* cl = T.lens + 300;
  for (int k = 0; k < 19; ++k) cl[k] = 0;
  for (int k = 0; k < hclen; ++k) { cl[PNG_CL_ORDER[k]] = (unsigned char)(pd_peek(zw, p) & 7u); p += 3; }
  int* count = T.lit.count;                                         // (scratch: the block's own codes are built later)
  unsigned* next = T.lit.first;
  int left = 1;
  for (int l = 0; l < 8; ++l) count[l] = 0;
  for (int k = 0; k < 19; ++k) count[cl[k]]++;
  unsigned code = 0;
  next[0] = 0;
  for (int l = 1; l <= 7; ++l) {
    code = (code + (unsigned)(l > 1 ? count[l - 1] : 0)) << 1;
    next[l] = code;
    left = (left << 1) - count[l];
  }
  if (left != 0) { T.stop = 1; T.bits |= PPST_PNG_S_LENGTHS; return; }       // (zlib: the code-length code must be complete)
  for (int k = 0; k < 128; ++k) T.cl_lut[k] = 0;
  for (int k = 0; k < 19; ++k) {
    const int l = cl[k];
    if (!l) continue;
    const unsigned rev = __brev(next[l]++) >> (32 - l);
    for (unsigned f = 0; f < (1u << (7 - l)); ++f) T.cl_lut[rev | (f << l)] = (unsigned short)((l << 8) | k);
  }
  const int total = hlit + hdist;
  int at = 0, prev = 0;
  while (at < total) {                                              // every pass adds at least one length: at most 316 passes
    if (p >= nbits) { T.stop = 1; T.bits |= PPST_PNG_S_STREAM; return; }
    v = pd_peek(zw, p);
    const unsigned e = T.cl_lut[v & 127u];
    if (!e) { T.stop = 1; T.bits |= PPST_PNG_S_LENGTHS; return; }
    const int l = (int)(e >> 8), s = (int)(e & 255u);
    p += (unsigned)l;
    v >>= l;
    int rep, val;
    if (s < 16) { rep = 1; val = s; }
    else if (s == 16) {
      if (at == 0) { T.stop = 1; T.bits |= PPST_PNG_S_LENGTHS; return; }
      rep = 3 + (int)(v & 3u); val = prev; p += 2;
    } else if (s == 17) { rep = 3 + (int)(v & 7u); val = 0; p += 3; }
    else { rep = 11 + (int)(v & 127u); val = 0; p += 7; }
    if (at + rep > total) { T.stop = 1; T.bits |= PPST_PNG_S_LENGTHS; return; }
    for (int k = 0; k < rep; ++k) T.lens[at < hlit ? at : 288 + (at - hlit)] = (unsigned char)val, ++at;
    prev = val;
  }
  if (p > nbits) { T.stop = 1; T.bits |= PPST_PNG_S_STREAM; return; }
  for (int k = hlit; k < 288; ++k) T.lens[k] = 0;
  for (int k = 288 + hdist; k < 320; ++k) T.lens[k] = 0;
  if (T.lens[256] == 0) { T.stop = 1; T.bits |= PPST_PNG_S_LENGTHS; return; }  // no end-of-block code
  T.nl = hlit; T.nd = hdist; T.p = p;
}

// Decodes from p until p reaches `end` or the block ends.  cnt: bytes put out; eob: 1 and p the bit behind the end-of-block
// code.  WRITE: raw / src from position `pos` of the stream on (every store checked against n), the status bits of what it met.
struct PdRun { unsigned p; int cnt, eob, bits; };
template <bool WRITE>
__device__ __forceinline__ PdRun pd_run(const PdTabs& T, const unsigned* __restrict__ zw, unsigned p, unsigned end, unsigned char* __restrict__ raw,
                                        int* __restrict__ src, int pos, int n) {
  PdRun o = {p, 0, 0, 0};
  while (p < end) {
    const PdTok t = pd_token(T, zw, p);
    p = t.p;
    if (t.kind == 2) { o.eob = 1; break; }
    if (t.kind == 3) { if (WRITE) o.bits |= PPST_PNG_S_CODE; continue; }
    if (t.kind == 0) {
      if (WRITE && pos < n) { raw[pos] = (unsigned char)t.len; src[pos] = pos; }
      ++pos; ++o.cnt;
      continue;
    }
    if (WRITE) {
      const bool far = t.dist > pos;
      if (far) o.bits |= PPST_PNG_S_DISTANCE;
      int back = 0;                                                 // i mod d, kept by wrapping: no division per byte
      for (int k = 0; k < t.len; ++k) {
        const int at = pos + k;
        if (at < n) {
          if (far) { raw[at] = 0; src[at] = at; }
          else src[at] = pos + back - t.dist;
        }
        back = back + 1 == t.dist ? 0 : back + 1;
      }
    }
    pos += t.len; o.cnt += t.len;
  }
  o.p = p;
  return o;
}

__global__ __launch_bounds__(PD_INF_T) void pd_inflate_kernel(const ppst_png_dec_image* __restrict__ descs, int B, void* work, int* __restrict__ status) {
  __shared__ PdTabs T;
  const int i = blockIdx.x, tid = threadIdx.x;
  const PdImg& im = open_plan<PdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  const unsigned char* zs = base + im.l.zs;
  const unsigned* zw = (const unsigned*)zs;
  unsigned char* raw = base + im.l.raw;
  int* src = (int*)(base + im.l.src);
  int* cnt = (int*)(base + im.l.cnt);
  const unsigned L = im.g.L, nbits = L * 8u, SB = im.g.SB;
  const int n = im.g.n;
  if (tid == 0) {
    T.stop = status[i] != 0;                                         // a bad chunk or header: the stream is not looked at
    T.bits = 0; T.p = 16; T.bfinal = 0;
  }
  if (tid < 29) { T.lbase[tid] = PD_LBASE[tid]; T.lext[tid] = PD_LEXT[tid]; }
  if (tid < 30) { T.dbase[tid] = PD_DBASE[tid]; T.dext[tid] = PD_DEXT[tid]; }
  __syncthreads();
  if (T.stop) return;
  int outpos = 0, max_rounds = 0;
  const unsigned max_blocks = nbits / 3u + 1u;
  for (unsigned blk = 0; blk < max_blocks; ++blk) {
    int tb = tid;                                                    // the thread number for the per-block steps, opaque for the
    asm volatile("" : "+v"(tb));                                     // same reason as in wg_scan
    if (tb == 0) pd_block_header(T, zw, zs, L);
    __syncthreads();
    if (T.stop) break;
    if (T.btype == 0) {
      const int len = (int)T.st_len;
      if (len > n - outpos) { if (tid == 0) T.bits |= PPST_PNG_S_STREAM; break; }
      for (int k = tid; k < len; k += PD_INF_T) { raw[outpos + k] = zs[T.st_at + k]; src[outpos + k] = outpos + k; }
      outpos += len;
    } else {
      // ---- the two codes of the block
      if (T.btype == 1 && tb < 320) T.lens[tb] = tb < 144 ? 8 : (tb < 256 ? 9 : (tb < 280 ? 7 : (tb < 288 ? 8 : 5)));
      for (int e = tb; e < 512; e += PD_INF_T) { T.lit.lut[e] = 0; T.dist.lut[e] = 0; }
      __syncthreads();
      if (tb == 0 && pd_code_counts(T.lit, T.lens, T.nl, false)) { T.stop = 1; atomicOr(&T.bits, PPST_PNG_S_LENGTHS); }
      if (tb == 64 && pd_code_counts(T.dist, T.lens + 288, T.nd, true)) { T.stop = 1; atomicOr(&T.bits, PPST_PNG_S_LENGTHS); }
      __syncthreads();
      if (T.stop) break;
      if (tb < 288) pd_code_fill(T.lit, T.lens, T.nl, tb);
      else if (tb < 320) pd_code_fill(T.dist, T.lens + 288, T.nd, tb - 288);
      __syncthreads();
      // ---- windows of one subsequence per lane, the same tables until the end-of-block code
      unsigned wstart = T.p, entry0 = T.p;
      bool fault = false;
      const unsigned max_windows = (nbits - min(nbits, wstart)) / (SB * PD_INF_T) + 2u;
      for (unsigned w = 0; w < max_windows; ++w) {
        if (wstart >= nbits || entry0 >= nbits) { fault = true; break; }            // the bits end inside the block
        const unsigned nact = min((unsigned)PD_INF_T, (nbits - wstart + SB - 1) / SB);
        const bool active = (unsigned)tid < nact;
        const unsigned sb = wstart + (unsigned)tid * SB, end = min(nbits, sb + SB);
        unsigned entry = tid == 0 ? entry0 : sb;
        bool dirty = active;
        int mine = 0, eob = 0;
        unsigned eob_p = 0;
        if (tid == 0) T.eob_lane = PD_INF_T;
        int rounds = 0;
        for (;;) {
          if (dirty) {
            const PdRun x = pd_run<false>(T, zw, entry, end, nullptr, nullptr, 0, 0);
            mine = x.cnt; eob = x.eob; eob_p = x.p;
            T.X[tid] = x.eob ? PD_DEAD : x.p;
          }
          __syncthreads();
          ++rounds;
          int changed = 0;
          dirty = false;
          if (active && tid > 0) {
            const unsigned pe = T.X[tid - 1];
            if (pe != entry) {
              entry = pe;
              // a lane behind the block's end has nothing to decode and nothing to hand on: it takes no part in the fixed point
              // (its exit stays what it was; everything behind the first end-of-block is dropped below)
              if (pe == PD_DEAD) { mine = 0; eob = 0; }
              else { dirty = true; changed = 1; }
            }
          }
          if (!__syncthreads_or(changed)) break;
          if (rounds > PD_INF_T) break;                                             // (never: after round r the first r entries are final)
        }
        max_rounds = max(max_rounds, rounds);
        // the chain is exact up to the first lane that met an end-of-block; lanes behind it hold leftovers of wrong guesses
        if (active && eob) atomicMin(&T.eob_lane, tid);
        __syncthreads();
        const bool live = active && tid <= T.eob_lane;
        int total;
        const int pre = wg_scan<PD_INF_T, true>(live ? mine : 0, total, T.wt, 0);
        if (tid == T.eob_lane) T.eob_p = eob_p;
        if (total > n - outpos) { if (tid == 0) T.bits |= PPST_PNG_S_STREAM; fault = true; }
        if (live && !fault) {
          const PdRun x = pd_run<true>(T, zw, entry, end, raw, src, outpos + pre, n);
          if (x.bits) atomicOr(&T.bits, x.bits);
        }
        outpos += total;
        __syncthreads();
        if (fault) break;
        if (T.eob_lane < PD_INF_T) break;
        entry0 = T.X[nact - 1];
        wstart += SB * PD_INF_T;
        __syncthreads();                                                            // X and eob_lane are rewritten by the next window
      }
      if (fault || T.eob_lane >= PD_INF_T) { if (tid == 0) T.bits |= PPST_PNG_S_STREAM; break; }
      __syncthreads();
      if (tid == 0) T.p = T.eob_p;
      __syncthreads();
    }
    if (T.bfinal) {
      if (tid == 0) cnt[PD_ROUNDS_MAX] = (int)T.p;
      break;
    }
    __syncthreads();                                                                // the next header rewrites what this block read
  }
  __syncthreads();
  if (tid == 0) {
    int bits = T.bits;
    if (!bits && (!T.bfinal || outpos != n)) bits |= PPST_PNG_S_STREAM;
    if (bits) atomicOr(&status[i], bits);
    atomicMax((int*)work + i, max_rounds);
  }
}

// ---------------------------------------------------------------------------------------------------------- back-references
// One round of src[i] <- src[src[i]], in place: every value ever stored in src[i] is an ancestor of i on its chain and literals
// are fixed points, so a racing read sees a valid ancestor that is no farther from the root.
__global__ __launch_bounds__(PD_T) void pd_jump_kernel(int B, void* work, const int* __restrict__ status, int round) {
  __shared__ int any;
  const int i = blockIdx.y;
  const PdImg& im = open_plan<PdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  int* cnt = (int*)(base + im.l.cnt);
  if (round >= im.g.jumps || status[i] != 0) return;                  // (a damaged stream may leave src undefined: not followed)
  if (round > 0 && cnt[round - 1] == 0) return;
  const int64_t i0 = (int64_t)blockIdx.x * (PD_T * 4);
  if (i0 >= im.g.n) return;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  int* src = (int*)(base + im.l.src);
  const int n = im.g.n;
  int changed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t e = i0 + k * PD_T + threadIdx.x;
    if (e < n) {
      const int a = src[e];
      if ((unsigned)a < (unsigned)n) {
        const int b = src[a];
        if (b != a && (unsigned)b < (unsigned)n) { src[e] = b; changed = 1; }
      }
    }
  }
  if (changed) any = 1;
  __syncthreads();
  if (threadIdx.x == 0 && any) atomicAdd(&cnt[round], 1);
}

__global__ __launch_bounds__(PD_T) void pd_resolve_kernel(int B, void* work, const int* __restrict__ status) {
  __shared__ unsigned sa, sb;
  const int i = blockIdx.y, tid = threadIdx.x;
  const PdImg& im = open_plan<PdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  if ((int)blockIdx.x >= im.g.nchunk || status[i] != 0) return;
  if (tid == 0) { sa = 0; sb = 0; }
  __syncthreads();
  const unsigned char* raw = base + im.l.raw;
  const int* src = (const int*)(base + im.l.src);
  unsigned char* stream = base + im.l.stream;
  const int n = im.g.n;
  const int c0 = (int)blockIdx.x * PD_CHUNK, m = min(PD_CHUNK, n - c0);   // this piece: bytes [c0, c0 + m)
  unsigned a = 0, b = 0;
  for (int k = 0; k < 16; ++k) {
    const int j = tid * 16 + k;
    if (j >= m) break;
    const int s = src[c0 + j];
    const unsigned v = (unsigned)s < (unsigned)n ? raw[s] : 0u;
    stream[c0 + j] = (unsigned char)v;
    a += v;
    b += (unsigned)(m - j) * v;                                        // <= 16 * 4096 * 255
  }
  if (a) { atomicAdd(&sa, a); atomicAdd(&sb, b % PNG_ADLER); }           // <= 256 * 65520
  __syncthreads();
  if (tid == 0) {
    unsigned* part = (unsigned*)(base + im.l.part);
    part[2 * blockIdx.x] = sa % PNG_ADLER;
    part[2 * blockIdx.x + 1] = sb % PNG_ADLER;
  }
}

// ----------------------------------------------------------------------------------------------------------------- unfilter
__device__ __forceinline__ unsigned pd_load_px(const unsigned char* __restrict__ p, int C) {
  unsigned v = p[0];
  if (C >= 3) v |= ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
  if (C == 4) v |= (unsigned)p[3] << 24;
  return v;
}

// Rows in bands of 64: lane l of a wave owns row 64 band + l and is one pixel behind lane l - 1, whose last pixel -- the one above
// -- it takes by a cross-lane move; the pixel above and to the left is the one it took a step earlier.  A band runs in pieces of
// 64 steps; piece k of band b runs in round 2 b + k, when the last row of band b - 1 is 64 pixels ahead: lane 0 reads that row,
// and every lane its own first neighbours, from the rows already undone in place.  Waves take the bands in turn; a barrier
// closes every round.
__global__ __launch_bounds__(PD_INF_T) void pd_unfilter_kernel(const ppst_png_dec_image* __restrict__ descs, int B, void* work,
                                                               unsigned char* __restrict__ out_u8, int* __restrict__ status) {
  __shared__ int skip;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PdImg& im = open_plan<PdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  const ppst_png_dec_image& d = descs[i];
  if (tid == 0) skip = status[i] != 0;
  __syncthreads();
  if (skip) return;
  unsigned char* st = base + im.l.stream;
  const int H = im.g.H, W = im.g.W, C = im.g.C, row = im.g.row, co = im.g.cout;
  if (tid == 0) {                                                    // Adler-32 of the stream against the four bytes behind the final block
    const unsigned* part = (const unsigned*)(base + im.l.part);
    const int* cnt = (const int*)(base + im.l.cnt);
    unsigned a = 1, b = 0;
    for (int c = 0; c < im.g.nchunk; ++c)
      adler_join(a, b, (unsigned)min(PD_CHUNK, im.g.n - c * PD_CHUNK), part[2 * c], part[2 * c + 1]);
    const unsigned at = ((unsigned)cnt[PD_ROUNDS_MAX] + 7u) >> 3;
    const unsigned char* zs = base + im.l.zs;
    bool bad = at + 4 > im.g.L;
    if (!bad) bad = ((b << 16) | a) != (((unsigned)zs[at] << 24) | ((unsigned)zs[at + 1] << 16) | ((unsigned)zs[at + 2] << 8) | (unsigned)zs[at + 3]);
    if (bad) atomicOr(&status[i], PPST_PNG_S_ADLER);
  }
  const int NB = (H + 63) >> 6, K = (W + 126) >> 6, nsteps = 2 * (NB - 1) + K;
  unsigned char* out = out_u8 + d.out_off;
  int bad_filter = 0;
  for (int s = 0; s < nsteps; ++s) {
    for (int b = wave; b < NB; b += PD_INF_T / 64) {
      const int k = s - 2 * b;
      if (k < 0) break;
      if (k >= K) continue;
      const int y = b * 64 + lane;
      const bool valid = y < H;
      unsigned char* cur = st + (int64_t)(valid ? y : 0) * row + 1;
      const unsigned char* above = cur - row;                          // (read for y > 0 only)
      const int ft = valid ? cur[-1] : 0;
      bad_filter |= ft > 4;
      const int x0 = k * 64 - lane;
      unsigned left = 0, ul = 0;
      if (valid && x0 >= 1 && x0 - 1 < W) {
        left = pd_load_px(cur + (int64_t)(x0 - 1) * C, C);
        if (y > 0) ul = pd_load_px(above + (int64_t)(x0 - 1) * C, C);
      }
      for (int t = 0; t < 64; ++t) {
        const int x = x0 + t;
        unsigned up = __shfl_up(left, 1, 64);
        const bool in = valid && x >= 0 && x < W;
        if (lane == 0) up = (in && y > 0) ? pd_load_px(above + (int64_t)x * C, C) : 0u;
        if (in) {
          const unsigned f = pd_load_px(cur + (int64_t)x * C, C);
          unsigned r = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int fa = (int)((left >> (8 * c)) & 255u), fb = (int)((up >> (8 * c)) & 255u), fc = (int)((ul >> (8 * c)) & 255u);
            const int add = ft == 1 ? fa : (ft == 2 ? fb : (ft == 3 ? (fa + fb) >> 1 : (ft == 4 ? png_paeth(fa, fb, fc) : 0)));
            r |= ((((f >> (8 * c)) & 255u) + (unsigned)add) & 255u) << (8 * c);
          }
          unsigned char* q = cur + (int64_t)x * C;
          q[0] = (unsigned char)r;
          if (C >= 3) { q[1] = (unsigned char)(r >> 8); q[2] = (unsigned char)(r >> 16); }
          if (C == 4) q[3] = (unsigned char)(r >> 24);
          const int xo = d.mirror ? W - 1 - x : x;
          unsigned char* o = out + ((int64_t)y * W + xo) * co;
          o[0] = (unsigned char)r;
          if (co >= 3) {
            o[1] = (unsigned char)(C == 1 ? r : r >> 8);
            o[2] = (unsigned char)(C == 1 ? r : r >> 16);
          }
          if (co == 4) o[3] = (unsigned char)(r >> 24);
          ul = up;
          left = r;
        }
      }
    }
    __syncthreads();
  }
  if (bad_filter) atomicOr(&status[i], PPST_PNG_S_FILTER);
}

// --------------------------------------------------------------------------------------------------------------------- host
// a descriptor ppst_png_parse can have made (the kernels index with these fields)
static bool pd_valid(const ppst_png_dec_image& d) {
  if (d.H < 1 || d.W < 1) return false;
  if (!((d.colour == 0 && d.channels == 1) || (d.colour == 2 && d.channels == 3) || (d.colour == 6 && d.channels == 4))) return false;
  const uint64_t row = 1u + (uint64_t)d.W * (uint64_t)d.channels;
  if (row >= 0x80000000ull || (uint64_t)d.H * row >= 0x80000000ull) return false;
  if (d.file_len < 0 || d.file_len >= 0x10000000ll || d.idat_bytes < 0 || d.idat_bytes > d.file_len) return false;
  if (d.nspans < 1 || d.nidat < 1 || d.first_idat < 0 || (int64_t)d.first_idat + d.nidat > d.nspans) return false;
  if (d.file_off < 0 || d.out_off < 0 || d.span_off < 0) return false;
  return true;
}

static bool pd_sw_ok(int sw) { return sw == 0 || (sw >= 2 && sw <= PD_SUBSEQ_MAX); }

extern "C" int64_t ppst_png_decode_ws(const ppst_png_dec_image* descs, int B, int subseq_words) {
  if (B < 0 || B > 65535 || !pd_sw_ok(subseq_words)) return PPST_EINVAL;
  if (B > 0 && !descs) return PPST_ENULL;
  int64_t total = head_bytes<PdImg>(B > 0 ? B : 1);
  for (int i = 0; i < B; ++i) {
    if (!pd_valid(descs[i])) return PPST_EINVAL;
    PdImg im;
    codec_fill(descs[i], subseq_words, &im);
    total += im.l.total;
  }
  return total;
}

extern "C" int ppst_png_decode(const void* files, int64_t files_bytes, const ppst_png_dec_image* descs_host, const void* descs_dev,
                               const void* spans_dev, void* out_u8, int64_t out_bytes, void* status, int B, int subseq_words, void* work,
                               void* stream) {
  if (B < 0 || B > 65535 || !pd_sw_ok(subseq_words) || files_bytes < 0 || out_bytes < 0) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!descs_host) return PPST_ENULL;
  int max_spans = 1, max_jumps = 1;
  int64_t max_n = 1;
  for (int i = 0; i < B; ++i) {
    const ppst_png_dec_image& d = descs_host[i];
    if (!pd_valid(d)) return PPST_EINVAL;
    PdGeom g;
    pd_geom(d, subseq_words, &g);
    if (d.file_off > files_bytes || d.file_len > files_bytes - d.file_off) return PPST_EINVAL;
    if (d.out_off > out_bytes || (int64_t)d.H * d.W * g.cout > out_bytes - d.out_off) return PPST_EINVAL;
    if (d.nspans > max_spans) max_spans = d.nspans;
    if (g.jumps > max_jumps) max_jumps = g.jumps;
    if (g.n > max_n) max_n = g.n;
  }
  if (!files || !descs_dev || !spans_dev || !out_u8 || !status || !work) return PPST_ENULL;
  if (((uintptr_t)work | (uintptr_t)out_u8 | (uintptr_t)descs_dev | (uintptr_t)spans_dev) & 15) return PPST_EINVAL;
  hipStream_t st = as_stream(stream);
  const ppst_png_dec_image* dd = (const ppst_png_dec_image*)descs_dev;
  const ppst_png_span* sp = (const ppst_png_span*)spans_dev;
  const unsigned char* by = (const unsigned char*)files;
  int* stt = (int*)status;
  static_assert(sizeof(PdTabs) <= 16 * 1024, "the inflate workgroup's tables");
  static_assert(PD_ROUNDS_MAX >= 33, "one counter per pointer-jumping round");
  PPST_LAUNCH(plan_kernel<PdImg>, dim3(1), dim3(256), 0, st, dd, B, subseq_words, work, stt);
  PPST_LAUNCH(pd_offsets_kernel, dim3((unsigned)B), dim3(PD_T), 0, st, by, dd, sp, B, work, stt);
  PPST_LAUNCH(pd_chunk_kernel, dim3((unsigned)max_spans, (unsigned)B), dim3(PD_T), 0, st, by, dd, sp, B, work, stt);
  PPST_LAUNCH(pd_inflate_kernel, dim3((unsigned)B), dim3(PD_INF_T), 0, st, dd, B, work, stt);
  const unsigned jump_blocks = (unsigned)cdiv64(max_n, PD_T * 4);
  for (int r = 0; r < max_jumps; ++r) PPST_LAUNCH(pd_jump_kernel, dim3(jump_blocks, (unsigned)B), dim3(PD_T), 0, st, B, work, stt, r);
  PPST_LAUNCH(pd_resolve_kernel, dim3((unsigned)cdiv64(max_n, PD_CHUNK), (unsigned)B), dim3(PD_T), 0, st, B, work, stt);
  PPST_LAUNCH(pd_unfilter_kernel, dim3((unsigned)B), dim3(PD_INF_T), 0, st, dd, B, work, (unsigned char*)out_u8, stt);
  return PPST_LAUNCH_CHECK();
}
