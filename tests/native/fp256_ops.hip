// Every primitive of starks_amd/csrc/fp256.cuh, elementwise, on the device and on the host: the harness of tests/test_field_arith_host.py
// (host mode) and tests/test_gpu_field_arith.py (device mode, with the header's inline asm and with -DSHK_NO_ADD_ASM).  Operands and
// results are little-endian u32 limbs; the tests compare them with exact integers.
//   fp256_ops --device|--host JOBS      JOBS: one job per line, "op n grid block in out": read n records of the op's operand size
//   from the file `in`, write n result records to `out`.  --device runs one kernel launch of `grid` blocks of `block` threads, one
//   element per thread; --host runs a plain loop (grid and block are ignored).
// Records, in u32 words (operand -> result):
//   add sub mul eqcanon: a[8] b[8] -> 8 (eqcanon: 1 word, 0 or 1)     neg sqr mulaa div4 canon inv: a[8] -> 8
//   mul2: x[8] w[8] w128[8] -> 8            mulwide: a[8] b[8] -> 16    mul2wide: x[8] w[8] w128[8] -> 13
//   redwide: t[16] -> 8                     red13: t[13] -> 8           pow: a[8] e[2] (u64) -> 8
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "fp256.cuh"

enum { OP_ADD, OP_SUB, OP_NEG, OP_MUL, OP_SQR, OP_MULAA, OP_MUL2, OP_MULWIDE, OP_MUL2WIDE, OP_REDWIDE, OP_RED13, OP_DIV4, OP_CANON,
       OP_EQCANON, OP_POW, OP_INV, OP_COUNT };

static const char* const OP_NAMES[OP_COUNT] = {"add", "sub", "neg", "mul", "sqr", "mulaa", "mul2", "mulwide", "mul2wide", "redwide",
                                               "red13", "div4", "canon", "eqcanon", "pow", "inv"};
constexpr int IN_WORDS[OP_COUNT] = {16, 16, 8, 16, 8, 8, 24, 16, 24, 16, 13, 8, 8, 16, 10, 8};
constexpr int OUT_WORDS[OP_COUNT] = {8, 8, 8, 8, 8, 8, 8, 16, 13, 8, 8, 8, 8, 1, 8, 8};

FP_HD fp ld(const uint32_t* x) {
  fp r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = x[i];
  return r;
}
FP_HD void st(const fp& a, uint32_t* y) {
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = a.v[i];
}

// one element: x = its operand record, y = its result record
template <int OP>
FP_HD void apply(const uint32_t* x, uint32_t* y) {
  if constexpr (OP == OP_ADD) {
    st(fp_add(ld(x), ld(x + 8)), y);
  } else if constexpr (OP == OP_SUB) {
    st(fp_sub(ld(x), ld(x + 8)), y);
  } else if constexpr (OP == OP_NEG) {
    st(fp_neg(ld(x)), y);
  } else if constexpr (OP == OP_MUL) {
    st(fp_mul(ld(x), ld(x + 8)), y);
  } else if constexpr (OP == OP_SQR) {
    st(fp_sqr(ld(x)), y);
  } else if constexpr (OP == OP_MULAA) {  // both operands the same object: the asm's early-clobber outputs must not overlap it
    const fp a = ld(x);
    st(fp_mul(a, a), y);
  } else if constexpr (OP == OP_MUL2) {
    fp2 w;
    w.w = ld(x + 8);
    w.w128 = ld(x + 16);
    st(fp_mul2(ld(x), w), y);
  } else if constexpr (OP == OP_MULWIDE) {
    const fp a = ld(x), b = ld(x + 8);
#if defined(__HIP_DEVICE_COMPILE__)
    fp_mul_wide_asm(a.v, b.v, y);
#else
    fp_mul_wide(a.v, b.v, y);
#endif
  } else if constexpr (OP == OP_MUL2WIDE) {
    const fp a = ld(x), w = ld(x + 8), w128 = ld(x + 16);
#if defined(__HIP_DEVICE_COMPILE__)
    fp_mul2_wide_asm(a.v, w.v, w128.v, y);
#else
    fp_mul2_wide(a.v, w.v, w128.v, y);
#endif
  } else if constexpr (OP == OP_REDWIDE) {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = x[i];
    st(fp_reduce_wide(t), y);
  } else if constexpr (OP == OP_RED13) {
    uint32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) t[i] = x[i];
    st(fp_reduce_13(t), y);
  } else if constexpr (OP == OP_DIV4) {
    st(fp_div4(ld(x)), y);
  } else if constexpr (OP == OP_CANON) {
    st(fp_canon(ld(x)), y);
  } else if constexpr (OP == OP_EQCANON) {
    y[0] = fp_eq_canon(fp_canon(ld(x)), fp_canon(ld(x + 8))) ? 1u : 0u;
  } else if constexpr (OP == OP_POW) {
    st(fp_pow_u64(ld(x), (uint64_t)x[8] | ((uint64_t)x[9] << 32)), y);
  } else if constexpr (OP == OP_INV) {
    st(fp_inv(ld(x)), y);
  }
}

template <int OP>
__global__ void op_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int IW = IN_WORDS[OP], OW = OUT_WORDS[OP];
  uint32_t x[IW], y[OW];
#pragma unroll
  for (int k = 0; k < IW; ++k) x[k] = in[(size_t)i * IW + k];
  apply<OP>(x, y);
#pragma unroll
  for (int k = 0; k < OW; ++k) out[(size_t)i * OW + k] = y[k];
}

template <int OP>
static void run_host(const uint32_t* in, uint32_t* out, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) apply<OP>(in + (size_t)i * IN_WORDS[OP], out + (size_t)i * OUT_WORDS[OP]);
}
template <int OP>
static void launch(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t grid, uint32_t block) {
  hipLaunchKernelGGL(op_kernel<OP>, dim3(grid), dim3(block), 0, 0, in, out, n);
}

typedef void (*HostFn)(const uint32_t*, uint32_t*, uint32_t);
typedef void (*LaunchFn)(const uint32_t*, uint32_t*, uint32_t, uint32_t, uint32_t);
template <int... K>
struct Table {
  static constexpr HostFn host[sizeof...(K)] = {run_host<K>...};
  static constexpr LaunchFn dev[sizeof...(K)] = {launch<K>...};
};
typedef Table<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15> Ops;
static_assert(OP_COUNT == 16, "one table entry per op");

static bool slurp(const char* path, std::vector<uint32_t>& v, size_t words) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  v.assign(words, 0);
  const size_t got = fread(v.data(), 4, words, f);
  const bool at_end = fgetc(f) == EOF;
  fclose(f);
  return got == words && at_end;  // exactly `words` words: no more, no fewer
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
  if (device) {
    uint32_t *din = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc(&din, in.size() * 4));
    HIP_OK(hipMalloc(&dout, out.size() * 4));
    HIP_OK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xa5, out.size() * 4));  // a lane that stores nothing shows up as a wrong value
    Ops::dev[op](din, dout, n, grid, block);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(din));
    HIP_OK(hipFree(dout));
  } else {
    Ops::host[op](in.data(), out.data(), n);
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
    if (op == OP_COUNT || n == 0 || n >= (1ull << 31)) {
      fprintf(stderr, "bad job: %s %llu\n", name, n);
      rc = 2;
      break;
    }
    // every element needs a thread, and thread indices are 32-bit
    if (device && (block == 0 || block > 1024 || grid == 0 || grid * block < n || grid * block >= (1ull << 32))) {
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
