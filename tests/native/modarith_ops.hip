// Every primitive of starks_amd/csrc/fpm.cuh and starks_amd/csrc/fp64m.cuh (Montgomery arithmetic with a run-time modulus) and the
// small functions the items headers build on them, elementwise, on the device and on the host: the harness of
// tests/test_modarith_host.py (host mode) and tests/test_gpu_modarith.py (device mode).  The tests compare the results with exact
// integers (tests/modarith_cases.py).
//   modarith_ops --device|--host JOBS      JOBS: one job per line, "op n grid block in out": read the modulus and n records of the
//   op's operand size from the file `in`, write n result records to `out`.  --device runs one kernel launch of `grid` blocks of
//   `block` threads, one element per thread; --host runs a plain loop (grid and block are ignored).
// The modulus is the first record of `in`: 32 bytes (8 x u32 little-endian limbs) for the fpm_ ops, one 8-byte word for the f64_ ops.
// The fpm_mod / f64_mod block is built here on the host (fpm_mod_init / f64_mod_init) and handed to the kernel by value as a kernel
// argument, as every library kernel takes it.  An even modulus or one below 3 is refused.
// fpm_ records are whole 32-byte values (8 x u32 little-endian limbs), loaded and stored with mn_ld / mn_st (operand -> result):
//   add sub mul mulp msub: a b -> 1        neg sqr to_mont from_mont canon half coef inv1: a -> 1
//   pow: a e (the low 64 bits of e) -> 1    pow_limbs: a e (256 bits) -> 1    below_p: a -> 1 (the value 0 or 1)
//   wire: w -> fpm_from_wire_words(w), fpm_to_wire_words of that
// f64_ records are 8-byte words:
//   add sub mul pow mulp msub: a b -> 1     neg sqr to_mont from_mont canon half coef inv1: a -> 1
//   from_limbs: 4 words (8 x u32 limbs) -> 1                                  wire: x -> 4 words (m6_wire_words' 8 x u32)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fp64m.cuh"
#include "fpm.cuh"
#include "mod64eval_items.cuh"  // m6e_coef; mod64poly_items.cuh: m6p_mulp, m6p_sub, m6p_inv1
#include "mod64fri_items.cuh"   // m6_half, m6_wire_words
#include "modeval_items.cuh"    // me_below_p, me_coef; modpoly_items.cuh: mp_mulp, mp_sub, mp_inv1; modstark_items.cuh: fpm_pow_limbs;
                                // modfri_items.cuh: mf_half; modntt_items.cuh: mn_ld, mn_st

enum { M_ADD, M_SUB, M_NEG, M_MUL, M_SQR, M_TO_MONT, M_FROM_MONT, M_CANON, M_POW, M_WIRE, M_POW_LIMBS, M_HALF, M_BELOW_P, M_COEF, M_MULP,
       M_MSUB, M_INV1, M_COUNT };
enum { W_ADD, W_SUB, W_NEG, W_MUL, W_SQR, W_TO_MONT, W_FROM_MONT, W_CANON, W_POW, W_FROM_LIMBS, W_HALF, W_WIRE, W_COEF, W_MULP, W_MSUB,
       W_INV1, W_COUNT };

static const char* const M_NAMES[M_COUNT] = {"fpm_add",  "fpm_sub",       "fpm_neg",  "fpm_mul",     "fpm_sqr",  "fpm_to_mont",
                                             "fpm_from_mont", "fpm_canon", "fpm_pow",  "fpm_wire",    "fpm_pow_limbs", "fpm_half",
                                             "fpm_below_p",   "fpm_coef",  "fpm_mulp", "fpm_msub",    "fpm_inv1"};
static const char* const W_NAMES[W_COUNT] = {"f64_add",  "f64_sub",   "f64_neg", "f64_mul",        "f64_sqr",  "f64_to_mont", "f64_from_mont",
                                             "f64_canon", "f64_pow",  "f64_from_limbs", "f64_half", "f64_wire", "f64_coef",    "f64_mulp",
                                             "f64_msub",  "f64_inv1"};
// record sizes: fpm_ ops in 32-byte values, f64_ ops in 8-byte words
constexpr int M_IN[M_COUNT] = {2, 2, 1, 2, 1, 1, 1, 1, 2, 1, 2, 1, 1, 1, 2, 2, 1};
constexpr int M_OUT[M_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1};
constexpr int W_IN[W_COUNT] = {2, 2, 1, 2, 1, 1, 1, 1, 2, 4, 1, 1, 1, 2, 2, 1};
constexpr int W_OUT[W_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 4, 1, 1, 1, 1};

// one element over fpm: x = its operand record, y = its result record; pm2 = p - 2 (ms_pm2), what the library hands mp_inv1
template <int OP>
FPM_HD void apply_m(const fpm* x, fpm* y, const fpm_mod& M, const fpm& pm2) {
  const fpm a = mn_ld(x);
  if constexpr (OP == M_ADD) {
    mn_st(y, fpm_add(a, mn_ld(x + 1), M));
  } else if constexpr (OP == M_SUB) {
    mn_st(y, fpm_sub(a, mn_ld(x + 1), M));
  } else if constexpr (OP == M_NEG) {
    mn_st(y, fpm_neg(a, M));
  } else if constexpr (OP == M_MUL) {
    mn_st(y, fpm_mul(a, mn_ld(x + 1), M));
  } else if constexpr (OP == M_SQR) {  // both arguments the same object
    mn_st(y, fpm_mul(a, a, M));
  } else if constexpr (OP == M_TO_MONT) {
    mn_st(y, fpm_to_mont(a, M));
  } else if constexpr (OP == M_FROM_MONT) {
    mn_st(y, fpm_from_mont(a, M));
  } else if constexpr (OP == M_CANON) {
    mn_st(y, fpm_canon(a, M));
  } else if constexpr (OP == M_POW) {
    const fpm e = mn_ld(x + 1);
    mn_st(y, fpm_pow(a, (uint64_t)e.v[0] | ((uint64_t)e.v[1] << 32), M));
  } else if constexpr (OP == M_WIRE) {
    const fpm v = fpm_from_wire_words(a.v);
    fpm w;
    fpm_to_wire_words(v, w.v);
    mn_st(y, v);
    mn_st(y + 1, w);
  } else if constexpr (OP == M_POW_LIMBS) {
    const fpm e = mn_ld(x + 1);
    mn_st(y, fpm_pow_limbs(a, e.v, M));
  } else if constexpr (OP == M_HALF) {
    mn_st(y, mf_half(a, M));
  } else if constexpr (OP == M_BELOW_P) {
    mn_st(y, fpm_from_u32(me_below_p(a, M) ? 1u : 0u));
  } else if constexpr (OP == M_COEF) {
    mn_st(y, me_coef(a, M));
  } else if constexpr (OP == M_MULP) {
    mn_st(y, mp_mulp(a, mn_ld(x + 1), M));
  } else if constexpr (OP == M_MSUB) {
    mn_st(y, mp_sub(a, mn_ld(x + 1), M));
  } else if constexpr (OP == M_INV1) {
    mn_st(y, mp_inv1(a, pm2, M));
  }
}

// one element over packed words
template <int OP>
F64_HD void apply_w(const uint64_t* x, uint64_t* y, const f64_mod& M) {
  const uint64_t a = x[0];
  if constexpr (OP == W_ADD) {
    y[0] = f64_add(a, x[1], M);
  } else if constexpr (OP == W_SUB) {
    y[0] = f64_sub(a, x[1], M);
  } else if constexpr (OP == W_NEG) {
    y[0] = f64_neg(a, M);
  } else if constexpr (OP == W_MUL) {
    y[0] = f64_mul(a, x[1], M);
  } else if constexpr (OP == W_SQR) {
    y[0] = f64_mul(a, a, M);
  } else if constexpr (OP == W_TO_MONT) {
    y[0] = f64_to_mont(a, M);
  } else if constexpr (OP == W_FROM_MONT) {
    y[0] = f64_from_mont(a, M);
  } else if constexpr (OP == W_CANON) {
    y[0] = f64_canon(a, M);
  } else if constexpr (OP == W_POW) {
    y[0] = f64_pow(a, x[1], M);
  } else if constexpr (OP == W_FROM_LIMBS) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[2 * i] = (uint32_t)x[i];
      w[2 * i + 1] = (uint32_t)(x[i] >> 32);
    }
    y[0] = f64_from_limbs(w, M);
  } else if constexpr (OP == W_HALF) {
    y[0] = m6_half(a, M);
  } else if constexpr (OP == W_WIRE) {
    uint32_t w[8];
    m6_wire_words(a, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  } else if constexpr (OP == W_COEF) {
    y[0] = m6e_coef(a, M);
  } else if constexpr (OP == W_MULP) {
    y[0] = m6p_mulp(a, x[1], M);
  } else if constexpr (OP == W_MSUB) {
    y[0] = m6p_sub(a, x[1], M);
  } else if constexpr (OP == W_INV1) {
    y[0] = m6p_inv1(a, M);
  }
}

template <int OP>
__global__ void m_kernel(const fpm* __restrict__ in, fpm* __restrict__ out, uint32_t n, fpm_mod M, fpm pm2) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  apply_m<OP>(in + (size_t)i * M_IN[OP], out + (size_t)i * M_OUT[OP], M, pm2);
}
template <int OP>
__global__ void w_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t n, f64_mod M) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int IW = W_IN[OP], OW = W_OUT[OP];
  uint64_t x[IW], y[OW];
#pragma unroll
  for (int k = 0; k < IW; ++k) x[k] = in[(size_t)i * IW + k];
  apply_w<OP>(x, y, M);
#pragma unroll
  for (int k = 0; k < OW; ++k) out[(size_t)i * OW + k] = y[k];
}

template <int OP>
static void m_host(const fpm* in, fpm* out, uint32_t n, const fpm_mod& M, const fpm& pm2) {
  for (uint32_t i = 0; i < n; ++i) apply_m<OP>(in + (size_t)i * M_IN[OP], out + (size_t)i * M_OUT[OP], M, pm2);
}
template <int OP>
static void w_host(const uint64_t* in, uint64_t* out, uint32_t n, const f64_mod& M) {
  for (uint32_t i = 0; i < n; ++i) apply_w<OP>(in + (size_t)i * W_IN[OP], out + (size_t)i * W_OUT[OP], M);
}
template <int OP>
static void m_launch(const fpm* in, fpm* out, uint32_t n, uint32_t grid, uint32_t block, const fpm_mod& M, const fpm& pm2) {
  hipLaunchKernelGGL(m_kernel<OP>, dim3(grid), dim3(block), 0, 0, in, out, n, M, pm2);
}
template <int OP>
static void w_launch(const uint64_t* in, uint64_t* out, uint32_t n, uint32_t grid, uint32_t block, const f64_mod& M) {
  hipLaunchKernelGGL(w_kernel<OP>, dim3(grid), dim3(block), 0, 0, in, out, n, M);
}

typedef void (*MHostFn)(const fpm*, fpm*, uint32_t, const fpm_mod&, const fpm&);
typedef void (*MLaunchFn)(const fpm*, fpm*, uint32_t, uint32_t, uint32_t, const fpm_mod&, const fpm&);
typedef void (*WHostFn)(const uint64_t*, uint64_t*, uint32_t, const f64_mod&);
typedef void (*WLaunchFn)(const uint64_t*, uint64_t*, uint32_t, uint32_t, uint32_t, const f64_mod&);
template <int... K>
struct MTable {
  static constexpr MHostFn host[sizeof...(K)] = {m_host<K>...};
  static constexpr MLaunchFn dev[sizeof...(K)] = {m_launch<K>...};
};
template <int... K>
struct WTable {
  static constexpr WHostFn host[sizeof...(K)] = {w_host<K>...};
  static constexpr WLaunchFn dev[sizeof...(K)] = {w_launch<K>...};
};
typedef MTable<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16> MOps;
typedef WTable<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15> WOps;
static_assert(M_COUNT == 17 && W_COUNT == 16, "one table entry per op");

// the whole file: `head` bytes of modulus, then exactly `body` bytes of records
static bool slurp(const char* path, std::vector<uint8_t>& v, size_t head, size_t body) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  v.assign(head + body, 0);
  const size_t got = fread(v.data(), 1, head + body, f);
  const bool at_end = fgetc(f) == EOF;
  fclose(f);
  return got == head + body && at_end;
}

#define HIP_OK(x)                                             \
  do {                                                        \
    const hipError_t e_ = (x);                                \
    if (e_ != hipSuccess) {                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      return 3;                                               \
    }                                                         \
  } while (0)

// wide: an fpm_ op (index op of MOps), else an f64_ op (index op of WOps)
static int run_job(bool device, bool wide, int op, uint32_t n, uint32_t grid, uint32_t block, const char* inp, const char* outp) {
  const size_t unit = wide ? 32 : 8, head = unit;
  const size_t in_bytes = (size_t)n * unit * (wide ? M_IN[op] : W_IN[op]), out_bytes = (size_t)n * unit * (wide ? M_OUT[op] : W_OUT[op]);
  std::vector<uint8_t> file;
  if (!slurp(inp, file, head, in_bytes)) {
    fprintf(stderr, "%s: expected the modulus and exactly %u records of %zu bytes\n", inp, n, in_bytes / n);
    return 2;
  }
  // the records on their own, aligned for either element type
  std::vector<uint64_t> in((in_bytes + 7) / 8), out((out_bytes + 7) / 8);
  memcpy(in.data(), file.data() + head, in_bytes);
  fpm_mod M = {};
  fpm pm2 = fpm_zero();
  f64_mod W = {};
  if (wide) {
    uint8_t be[32];
    for (int i = 0; i < 32; ++i) be[i] = file[31 - i];  // little-endian limbs -> the big-endian wire bytes fpm_mod_init reads
    if (!fpm_mod_init(be, &M)) {
      fprintf(stderr, "%s: the modulus must be odd and at least 3\n", inp);
      return 2;
    }
    pm2 = ms_pm2(M);
  } else {
    uint64_t p;
    memcpy(&p, file.data(), 8);
    if (!f64_mod_init(p, &W)) {
      fprintf(stderr, "%s: the modulus must be odd and at least 3\n", inp);
      return 2;
    }
  }
  if (device) {
    void *din = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc(&din, in_bytes));
    HIP_OK(hipMalloc(&dout, out_bytes));
    HIP_OK(hipMemcpy(din, in.data(), in_bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xa5, out_bytes));  // a lane that stores nothing shows up as a wrong value
    if (wide) MOps::dev[op]((const fpm*)din, (fpm*)dout, n, grid, block, M, pm2);
    else WOps::dev[op]((const uint64_t*)din, (uint64_t*)dout, n, grid, block, W);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), dout, out_bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(din));
    HIP_OK(hipFree(dout));
  } else if (wide) {
    MOps::host[op]((const fpm*)in.data(), (fpm*)out.data(), n, M, pm2);
  } else {
    WOps::host[op](in.data(), out.data(), n, W);
  }
  FILE* f = fopen(outp, "wb");
  if (!f || fwrite(out.data(), 1, out_bytes, f) != out_bytes || fclose(f) != 0) {
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
    bool wide = true;
    while (op < M_COUNT && strcmp(M_NAMES[op], name)) ++op;
    if (op == M_COUNT) {
      wide = false;
      op = 0;
      while (op < W_COUNT && strcmp(W_NAMES[op], name)) ++op;
    }
    if ((!wide && op == W_COUNT) || n == 0 || n >= (1ull << 24)) {
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
    if ((rc = run_job(device, wide, op, (uint32_t)n, (uint32_t)grid, (uint32_t)block, inp, outp)) != 0) break;
    ++done;
  }
  fclose(jobs);
  printf("%d jobs\n", done);
  return rc;
}
