// Every form of starks_amd/csrc/blake2s.cuh, and sample_indices_quad, on the device and on the host: the harness of
// tests/test_blake2s_host.py (host mode) and tests/test_gpu_blake2s.py (device mode, in every build of the header's switches and of
// the generator's forms).  Messages and digests are the bytes the kernels store, as little-endian u32 words; the tests compare them
// with hashlib.blake2s and starks_amd.utils.get_pseudorandom_indices.
//   blake2s_ops --device|--host JOBS    JOBS: one job per line, "op n grid block in out", the protocol of fp256_ops.hip: read n records
//   of the op's input size from `in`, write n result records to `out`.  --device runs one launch of `grid` blocks of `block` threads;
//   --host runs a plain loop through the portable paths (b2_compress_cpp, vb_hash_two), for the ops that have one.
// Records, in u32 words (input -> result); one element per thread unless marked "per quad":
//   pair:  m[16]                                         -> b2_hash_pair<true>(m, m + 8)[8], b2_hash_pair<false>[8]
//   short: len, pad[15], m[16] (zero past len)           -> b2_hash_short<true>(m, len)[8], b2_hash_short<false>[8]
//   chain: k, pad[15], blocks[255][16] (k = 1..255)      -> k compressions, counter 64 (blk + 1), final on the last: <true>[8], <false>[8]
//   vbtwo: len, pad[7], a[216], b[216] (len = 32..864, multiple of 32)   -> vb_hash_two(a, b, len)[8]
//   quad (per quad, device only):  m[16], tcount, live, pad[2]           -> b2q_compress digest[8]; a quad with live = 0 does nothing
//   sample (per quad, device only, 64-thread blocks): entropy[8], modulus, count, exclude, pad -> ys[count], the rest untouched
// Output buffers start filled with 0xa5 bytes: a lane that stores nothing, or stores too much, shows up as a wrong record.  The
// sampler's modulus, count and exclude are those of the block's first quad (the call sites pass one value per launch); the harness
// refuses a job whose quads in one block differ there, or whose arguments the library refuses.  The device buffers of the per-quad
// ops cover whole blocks; after a sampler launch the records of the dead quads past n must still be all 0xa5 (exit status 4 if not).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "blake2s.cuh"
#include "verify_items.cuh"

enum { OP_PAIR, OP_SHORT, OP_CHAIN, OP_VBTWO, OP_QUAD, OP_SAMPLE, OP_COUNT };

static const char* const OP_NAMES[OP_COUNT] = {"pair", "short", "chain", "vbtwo", "quad", "sample"};
constexpr int CHAIN_MAX = 255, VB_MAX = 32 * 27, SAMPLE_MAX = 256;
constexpr int IN_WORDS[OP_COUNT] = {16, 32, 16 + 16 * CHAIN_MAX, 8 + 2 * VB_MAX / 4, 20, 12};
constexpr int OUT_WORDS[OP_COUNT] = {16, 16, 16, 8, 8, SAMPLE_MAX};
constexpr bool PER_QUAD[OP_COUNT] = {false, false, false, false, true, true};
constexpr uint32_t SENTINEL = 0xa5a5a5a5u;

template <int OP>
B2_HD void apply(const uint32_t* x, uint32_t* y) {
  if constexpr (OP == OP_PAIR) {
    const b2digest d1 = b2_hash_pair<true>(x, x + 8), d0 = b2_hash_pair<false>(x, x + 8);
    for (int i = 0; i < 8; ++i) y[i] = d1.h[i], y[8 + i] = d0.h[i];
  } else if constexpr (OP == OP_SHORT) {
    uint32_t m[16];
    for (int i = 0; i < 16; ++i) m[i] = x[16 + i];
    const b2digest d1 = b2_hash_short<true>(m, x[0]), d0 = b2_hash_short<false>(m, x[0]);
    for (int i = 0; i < 8; ++i) y[i] = d1.h[i], y[8 + i] = d0.h[i];
  } else if constexpr (OP == OP_CHAIN) {  // the call-site loop (merkle_packed_leaves_kernel, quotient_leaf_pair)
    const uint32_t k = x[0];
    uint32_t h1[8], h0[8];
    b2_init(h1);
    b2_init(h0);
    for (uint32_t blk = 0; blk < k; ++blk) {
      uint32_t m[16];
      for (int i = 0; i < 16; ++i) m[i] = x[16 + 16 * blk + i];
      b2_compress<true>(h1, m, 64 * (blk + 1), blk + 1 == k);
    }
    for (uint32_t blk = 0; blk < k; ++blk) {
      uint32_t m[16];
      for (int i = 0; i < 16; ++i) m[i] = x[16 + 16 * blk + i];
      b2_compress<false>(h0, m, 64 * (blk + 1), blk + 1 == k);
    }
    for (int i = 0; i < 8; ++i) y[i] = h1[i], y[8 + i] = h0[i];
  } else if constexpr (OP == OP_VBTWO) {
    vb_hash_two(reinterpret_cast<const uint8_t*>(x + 8), reinterpret_cast<const uint8_t*>(x + 8 + VB_MAX / 4), x[0], y);
  }
}

template <int OP>
__global__ void op_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int OW = OUT_WORDS[OP];
  uint32_t y[OW];
  apply<OP>(in + (size_t)i * IN_WORDS[OP], y);
#pragma unroll
  for (int k = 0; k < OW; ++k) out[(size_t)i * OW + k] = y[k];
}

// one 64-byte message per quad, launched as merkle_top_kernel launches: each live quad stores its block in its own LDS slot, the
// block syncs, and the quad compresses it with the addresses of b2q_addr_init
__global__ void quad_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  extern __shared__ __attribute__((aligned(16))) uint32_t slots[];  // 16 words per quad
  const uint32_t tid = threadIdx.x, quad = tid >> 2, q = tid & 3;
  const uint32_t g = blockIdx.x * (blockDim.x >> 2) + quad;
  const uint32_t* rec = in + (size_t)g * IN_WORDS[OP_QUAD];
  const bool live = g < n && rec[17] != 0;
  b2q_addr ad;
  b2q_addr_init(ad, quad * 64, q);
  if (live) {
#pragma unroll
    for (int k = 0; k < 4; ++k) slots[quad * 16 + 4 * q + k] = rec[4 * q + k];
  }
  __syncthreads();
  if (live) {
    uint32_t h_lo = 0, h_hi = 0;
    b2q_compress(ad, slots, q, rec[16], h_lo, h_hi);
    out[(size_t)g * 8 + q] = h_lo;
    out[(size_t)g * 8 + 4 + q] = h_hi;
  }
}

// sample_indices_kernel's shape: 16 quads per 64-thread block, quad b live while b < n; every buffer covers the whole last block
__global__ void __launch_bounds__(64) sample_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  __shared__ __attribute__((aligned(16))) uint32_t slots[16 * 16];
  const uint32_t b = blockIdx.x * 16 + (threadIdx.x >> 2);
  const uint32_t* p = in + (size_t)blockIdx.x * 16 * IN_WORDS[OP_SAMPLE] + 8;  // the block's first quad: modulus, count, exclude
  sample_indices_quad(slots, in + (size_t)b * IN_WORDS[OP_SAMPLE], b < n, p[0], p[1], p[2], out + (size_t)b * SAMPLE_MAX);
}

template <int OP>
static void run_host(const uint32_t* in, uint32_t* out, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) apply<OP>(in + (size_t)i * IN_WORDS[OP], out + (size_t)i * OUT_WORDS[OP]);
}
template <int OP>
static void launch(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t grid, uint32_t block) {
  if constexpr (OP == OP_QUAD)
    hipLaunchKernelGGL(quad_kernel, dim3(grid), dim3(block), block * 16, 0, in, out, n);
  else if constexpr (OP == OP_SAMPLE)
    hipLaunchKernelGGL(sample_kernel, dim3(grid), dim3(block), 0, 0, in, out, n);
  else
    hipLaunchKernelGGL(op_kernel<OP>, dim3(grid), dim3(block), 0, 0, in, out, n);
}

typedef void (*HostFn)(const uint32_t*, uint32_t*, uint32_t);
typedef void (*LaunchFn)(const uint32_t*, uint32_t*, uint32_t, uint32_t, uint32_t);
static const HostFn HOST[OP_COUNT] = {run_host<OP_PAIR>, run_host<OP_SHORT>, run_host<OP_CHAIN>, run_host<OP_VBTWO>, nullptr, nullptr};
static const LaunchFn DEV[OP_COUNT] = {launch<OP_PAIR>, launch<OP_SHORT>, launch<OP_CHAIN>, launch<OP_VBTWO>, launch<OP_QUAD>,
                                       launch<OP_SAMPLE>};

static bool slurp(const char* path, std::vector<uint32_t>& v, size_t words) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  v.assign(words, 0);
  const size_t got = fread(v.data(), 4, words, f);
  const bool at_end = fgetc(f) == EOF;
  fclose(f);
  return got == words && at_end;  // exactly `words` words: no more, no fewer
}

// every record within what the op takes (the kernels index by these values); for the sampler, also what the library accepts
static bool valid(int op, const uint32_t* x, const uint32_t* first) {
  switch (op) {
    case OP_SHORT: return x[0] <= 64;
    case OP_CHAIN: return x[0] >= 1 && x[0] <= (uint32_t)CHAIN_MAX;
    case OP_VBTWO: return x[0] >= 32 && x[0] <= (uint32_t)VB_MAX && x[0] % 32 == 0;
    case OP_QUAD: return x[16] <= 64 && x[17] <= 1;
    case OP_SAMPLE: {
      const uint32_t modulus = x[8], count = x[9], exclude = x[10];
      if (modulus >= (1u << 24) || count > (uint32_t)SAMPLE_MAX - 1 || exclude == 1) return false;
      const uint64_t real = exclude ? (uint64_t)modulus * (exclude - 1) / exclude : modulus;
      return real >= 1 && modulus == first[8] && count == first[9] && exclude == first[10];
    }
    default: return true;
  }
}

#define HIP_OK(x)                                                                 \
  do {                                                                            \
    const hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                     \
      return 3;                                                                   \
    }                                                                             \
  } while (0)

static int run_job(bool device, int op, uint32_t n, uint32_t grid, uint32_t block, const char* inp, const char* outp) {
  std::vector<uint32_t> in, out((size_t)n * OUT_WORDS[op]);
  if (!slurp(inp, in, (size_t)n * IN_WORDS[op])) {
    fprintf(stderr, "%s: expected exactly %u records of %d words\n", inp, n, IN_WORDS[op]);
    return 2;
  }
  const uint32_t per_block = op == OP_SAMPLE ? 16 : 1;
  for (uint32_t i = 0; i < n; ++i)
    if (!valid(op, &in[(size_t)i * IN_WORDS[op]], &in[(size_t)(i / per_block * per_block) * IN_WORDS[op]])) {
      fprintf(stderr, "%s: record %u is outside what %s takes\n", inp, i, OP_NAMES[op]);
      return 2;
    }
  if (device) {
    // the per-quad ops read and write whole blocks of quads: their buffers cover grid * block / 4 records, the ones past n zero
    const size_t recs = PER_QUAD[op] ? (size_t)grid * block / 4 : n;
    std::vector<uint32_t> all(recs * OUT_WORDS[op]);
    in.resize(recs * IN_WORDS[op], 0);
    uint32_t *din = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc(&din, in.size() * 4));
    HIP_OK(hipMalloc(&dout, all.size() * 4));
    HIP_OK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xa5, all.size() * 4));
    DEV[op](din, dout, n, grid, block);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(all.data(), dout, all.size() * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(din));
    HIP_OK(hipFree(dout));
    for (size_t i = out.size(); i < all.size(); ++i)
      if (all[i] != SENTINEL) {
        fprintf(stderr, "%s: quad %zu, past n = %u, wrote word %zu\n", OP_NAMES[op], i / OUT_WORDS[op], n, i % OUT_WORDS[op]);
        return 4;
      }
    memcpy(out.data(), all.data(), out.size() * 4);
  } else {
    HOST[op](in.data(), out.data(), n);
  }
  FILE* f = fopen(outp, "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) {
    fprintf(stderr, "%s: write failed\n", outp);
    return 2;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3 || (strcmp(argv[1], "--device") && strcmp(argv[1], "--host"))) {
    fprintf(stderr, "usage: %s --device|--host JOBS\n", argv[0]);
    return 2;
  }
  const bool device = !strcmp(argv[1], "--device");
  FILE* jobs = fopen(argv[2], "r");
  if (!jobs) {
    fprintf(stderr, "%s: cannot open\n", argv[2]);
    return 2;
  }
  char name[32], inp[4096], outp[4096];
  unsigned long long n, grid, block;
  int done = 0, rc = 0;
  while (fscanf(jobs, "%31s %llu %llu %llu %4095s %4095s", name, &n, &grid, &block, inp, outp) == 6) {
    int op = 0;
    while (op < OP_COUNT && strcmp(OP_NAMES[op], name)) ++op;
    if (op == OP_COUNT || n == 0 || n >= (1ull << 24) || (!device && !HOST[op])) {
      fprintf(stderr, "bad job: %s %llu (%s)\n", name, n, device ? "device" : "host");
      rc = 2;
      break;
    }
    // every element (every quad: four threads) needs its threads, and thread indices are 32-bit; the quad ops take whole quads, and
    // the sampler the 64-thread blocks its LDS array is sized for
    const unsigned long long threads = PER_QUAD[op] ? 4 * n : n;
    if (device && (block == 0 || block > 1024 || grid == 0 || grid * block < threads || grid * block >= (1ull << 32) ||
                   (PER_QUAD[op] && block % 4) || (op == OP_SAMPLE && block != 64))) {
      fprintf(stderr, "bad launch for %s: %llu elements, %llu x %llu threads\n", name, n, grid, block);
      rc = 2;
      break;
    }
    if ((rc = run_job(device, op, (uint32_t)n, (uint32_t)grid, (uint32_t)block, inp, outp)) != 0) break;
    ++done;
  }
  fclose(jobs);
  printf("%d jobs\n", done);
  return rc;
}
