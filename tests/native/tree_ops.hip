// Every Merkle tree form and the FRI fold of starks_amd/csrc/kernels.hip, called through its shk_* entry points: the harness of
// tests/test_trees_host.py (cross-compile, refusals) and tests/test_gpu_trees.py (every case of tests/tree_cases.py on the device).
// Built together with kernels.hip alone:  hipcc -O3 --offload-arch=gfx950 -std=c++17 -I starks_amd/csrc tree_ops.hip kernels.hip
//   tree_ops JOBS    JOBS: one job per line, "op n batch arg in out"; every line is checked before the first HIP call.
// Values in `in` are 32-byte wire elements (big-endian, possibly >= p); the limb forms load them through shk_wire_to_limb, so an
// unreduced value stays unreduced on the device.  The harness does no field arithmetic: every table and constant comes from `in`.
//   tree  n batch form     form = 2 raw + store: 3 (raw leaves), 1 (limb, leaf level stored), 0 (limb, leaf level not stored)
//         in: values [batch][n]            out: nodes [batch][2n][32 B]  -- shk_merkelize
//   packed n 1 k           in: evals [k][n]  out: nodes [n][32 B] then leaves [n][k][32 B]  -- shk_merkelize_packed
//   fold  n batch flags    flags: 1 = a hi table is given, 2 = the challenge is node 1 of per-batch trees (else special_x)
//         in: header u32[8] = log_n0, lb, round_shift, 0...; inv_i, special_x; lo [2^lb]; hi [2^(log_n0 - lb)] (flag 1);
//             node1 [batch] (flag 2, placed at node 1 of a [batch][2n] node buffer filled with 0xa5)
//         out: column [batch][n/4] in LIMB form (little-endian words, as the kernel stores it)  -- shk_fri_fold
//   foldtree               the same input; out: the column, then nodes [batch][2 n/4][32 B]  -- shk_fri_fold_and_tree
// Every output buffer starts as 0xa5 bytes and runs GUARD bytes past its end: what a form must not write (the leaf level of the
// forms that do not store it) reads back as 0xa5, and a guard byte that changed ends the run with status 4.  Status 2: a job the
// harness refuses (nothing is run and nothing written); 3: a HIP error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <string>
#include <vector>

#include "internal.hpp"

enum { OP_TREE, OP_PACKED, OP_FOLD, OP_FOLDTREE, OP_COUNT };
static const char* const OP_NAMES[OP_COUNT] = {"tree", "packed", "fold", "foldtree"};
constexpr size_t GUARD = 4096;
constexpr uint64_t MAX_ELEMS = 1ull << 24;  // values per job (batch * n, or k * n)
constexpr uint32_t MAX_BATCH = 65535;       // the kernels put the batch on blockIdx.y
constexpr uint32_t MAX_LOG_N0 = 26;
constexpr uint32_t MAX_K = 64;

struct Job {
  int op;
  uint64_t n, batch, arg;
  std::string in, out;
  uint32_t log_n0, lb, round_shift;  // fold forms
};

static bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

static bool read_file(const char* path, std::vector<uint8_t>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  struct stat st;
  if (fstat(fileno(f), &st) != 0) {
    fclose(f);
    return false;
  }
  v.resize((size_t)st.st_size);
  const bool ok = fread(v.data(), 1, v.size(), f) == v.size();
  fclose(f);
  return ok;
}

static long long file_size(const char* path) {
  struct stat st;
  return stat(path, &st) == 0 ? (long long)st.st_size : -1;
}

static uint64_t fold_in_bytes(const Job& j) {
  uint64_t b = 32 + 64 + (32ull << j.lb) + (j.arg & 1 ? 32ull << (j.log_n0 - j.lb) : 0) + 32 * j.n * j.batch;
  if (j.arg & 2) b += 32 * j.batch;
  return b;
}

// the checks of shk_merkelize / shk_merkelize_packed / shk_fri_fold_and_tree, the buffers' sizes, and the fold's arguments
static const char* refuse(Job& j) {
  if (!pow2(j.n) || j.n < 4) return "n must be a power of two >= 4";
  if (j.batch == 0 || j.batch > MAX_BATCH) return "batch must be 1 .. 65535";
  const long long sz = file_size(j.in.c_str());
  if (sz < 0) return "cannot read the input";
  switch (j.op) {
    case OP_TREE:
      if (j.arg != 0 && j.arg != 1 && j.arg != 3) return "tree form must be 0, 1 or 3";
      if (j.n * j.batch > MAX_ELEMS) return "too many values";
      if ((uint64_t)sz != 32 * j.n * j.batch) return "input is not batch * n values";
      return nullptr;
    case OP_PACKED:
      if (j.batch != 1) return "packed trees take batch 1";
      if (j.arg == 0 || j.arg > MAX_K) return "k must be 1 .. 64";
      if (j.n * j.arg > MAX_ELEMS) return "too many values";
      if ((uint64_t)sz != 32 * j.n * j.arg) return "input is not k * n values";
      return nullptr;
    default: {
      if (j.arg > 3) return "fold flags must be 0 .. 3";
      if (j.op == OP_FOLDTREE && j.n / 4 < 4) return "foldtree needs n/4 >= 4";
      if (j.n * j.batch > MAX_ELEMS) return "too many values";
      if (sz < 32) return "no fold header";
      uint32_t h[8];
      FILE* f = fopen(j.in.c_str(), "rb");
      const bool got = f && fread(h, 4, 8, f) == 8;
      if (f) fclose(f);
      if (!got) return "no fold header";
      j.log_n0 = h[0], j.lb = h[1], j.round_shift = h[2];
      if (h[3] || h[4] || h[5] || h[6] || h[7]) return "fold header words 3..7 must be 0";
      if (j.log_n0 > MAX_LOG_N0 || j.round_shift > j.log_n0 || j.lb > j.log_n0) return "fold table out of range";
      if ((j.n << j.round_shift) != (1ull << j.log_n0)) return "n << round_shift must be 2^log_n0";
      if (!(j.arg & 1) && j.lb != j.log_n0) return "without a hi table, lo must hold all 2^log_n0 powers";
      if ((uint64_t)sz != fold_in_bytes(j)) return "input size does not match the fold header";
      return nullptr;
    }
  }
}

#define HIP_OK(x)                                             \
  do {                                                        \
    const hipError_t e_ = (x);                                \
    if (e_ != hipSuccess) {                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      return 3;                                               \
    }                                                         \
  } while (0)

// a device output buffer of `bytes` followed by GUARD bytes, all 0xa5
static int alloc_out(size_t bytes, uint8_t** d) {
  HIP_OK(hipMalloc((void**)d, bytes + GUARD));
  HIP_OK(hipMemset(*d, 0xa5, bytes + GUARD));
  return 0;
}
static int alloc_in(const uint8_t* src, size_t bytes, uint8_t** d) {
  HIP_OK(hipMalloc((void**)d, bytes ? bytes : 32));
  if (bytes) HIP_OK(hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
// the buffer back to the host, its guard checked
static int fetch(const uint8_t* d, size_t bytes, std::vector<uint8_t>& out, const char* what) {
  std::vector<uint8_t> all(bytes + GUARD);
  HIP_OK(hipMemcpy(all.data(), d, all.size(), hipMemcpyDeviceToHost));
  for (size_t i = bytes; i < all.size(); ++i)
    if (all[i] != 0xa5) {
      fprintf(stderr, "%s: guard byte %zu past the end (%zu bytes) was written\n", what, i - bytes, bytes);
      return 4;
    }
  out.insert(out.end(), all.begin(), all.begin() + bytes);
  return 0;
}
// wire values -> a limb array on the device (shk_wire_to_limb keeps values >= p as they are)
static int to_limbs(const uint8_t* wire, uint64_t n, fp** d) {
  uint8_t* w = nullptr;
  int rc = alloc_in(wire, 32 * n, &w);
  if (rc) return rc;
  HIP_OK(hipMalloc((void**)d, 32 * (n ? n : 1)));
  HIP_OK(shk_wire_to_limb(w, *d, n, 0));
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipFree(w));
  return 0;
}

#define RC(x)              \
  do {                     \
    const int r_ = (x);    \
    if (r_) return r_;     \
  } while (0)

static int run_job(const Job& j, std::vector<uint8_t>& out) {
  std::vector<uint8_t> in;
  if (!read_file(j.in.c_str(), in)) {
    fprintf(stderr, "%s: cannot read\n", j.in.c_str());
    return 2;
  }
  const uint64_t n = j.n, batch = j.batch;
  if (j.op == OP_TREE) {
    const bool raw = j.arg & 2, store = j.arg & 1;
    const size_t nb = 2 * n * batch * 32;
    uint8_t* nodes = nullptr;
    RC(alloc_out(nb, &nodes));
    void* leaves = nullptr;
    if (raw) {
      uint8_t* w = nullptr;
      RC(alloc_in(in.data(), in.size(), &w));
      leaves = w;
    } else {
      fp* l = nullptr;
      RC(to_limbs(in.data(), n * batch, &l));
      leaves = l;
    }
    HIP_OK(shk_merkelize(leaves, raw, n, (uint32_t)batch, reinterpret_cast<uint32_t*>(nodes), 0, store));
    HIP_OK(hipDeviceSynchronize());
    RC(fetch(nodes, nb, out, "nodes"));
    HIP_OK(hipFree(leaves));
    HIP_OK(hipFree(nodes));
    return 0;
  }
  if (j.op == OP_PACKED) {
    const uint64_t k = j.arg;
    uint8_t *evals = nullptr, *nodes = nullptr, *leaves = nullptr;
    RC(alloc_in(in.data(), in.size(), &evals));
    RC(alloc_out(32 * n, &nodes));
    RC(alloc_out(32 * n * k, &leaves));
    HIP_OK(shk_merkelize_packed(evals, n, (uint32_t)k, leaves, reinterpret_cast<uint32_t*>(nodes), 0));
    HIP_OK(hipDeviceSynchronize());
    RC(fetch(nodes, 32 * n, out, "nodes"));
    RC(fetch(leaves, 32 * n * k, out, "leaves"));
    HIP_OK(hipFree(evals));
    HIP_OK(hipFree(nodes));
    HIP_OK(hipFree(leaves));
    return 0;
  }
  // fold, foldtree: header, inv_i, special_x, lo, hi, values, node1
  const uint8_t* p = in.data() + 32;
  FoldArgs fa;
  memset(&fa, 0, sizeof fa);
  uint32_t w[8];
  memcpy(w, p, 32);
  fa.inv_i = fp_from_wire_words(w);  // a byte-order change: the limb form of the wire value
  p += 32;
  uint8_t* sx = nullptr;
  RC(alloc_in(p, 32, &sx));
  p += 32;
  fp *lo = nullptr, *hi = nullptr, *vals = nullptr;
  RC(to_limbs(p, 1ull << j.lb, &lo));
  p += 32ull << j.lb;
  if (j.arg & 1) {
    RC(to_limbs(p, 1ull << (j.log_n0 - j.lb), &hi));
    p += 32ull << (j.log_n0 - j.lb);
  }
  RC(to_limbs(p, n * batch, &vals));
  p += 32 * n * batch;
  uint8_t* tnodes = nullptr;
  if (j.arg & 2) {  // trees of the values: only node 1 of each is read
    RC(alloc_out(2 * n * batch * 32, &tnodes));
    for (uint64_t b = 0; b < batch; ++b) HIP_OK(hipMemcpy(tnodes + (b * 2 * n + 1) * 32, p + 32 * b, 32, hipMemcpyHostToDevice));
  }
  const uint64_t q = n / 4;
  uint8_t *col = nullptr, *nodes2 = nullptr;
  RC(alloc_out(32 * q * batch, &col));
  fa.values = vals;
  fa.nodes = reinterpret_cast<const uint32_t*>(tnodes);
  fa.special_x = reinterpret_cast<const uint32_t*>(sx);
  fa.column = reinterpret_cast<fp*>(col);
  fa.n = n;
  fa.batch = (uint32_t)batch;
  fa.tw_lo = lo;
  fa.tw_hi = hi;
  fa.tw_lb = j.lb;
  fa.log_n0 = j.log_n0;
  fa.round_shift = j.round_shift;
  if (j.op == OP_FOLD) {
    HIP_OK(shk_fri_fold(fa, 0));
  } else {
    RC(alloc_out(2 * q * batch * 32, &nodes2));
    HIP_OK(shk_fri_fold_and_tree(fa, reinterpret_cast<uint32_t*>(nodes2), 0));
  }
  HIP_OK(hipDeviceSynchronize());
  RC(fetch(col, 32 * q * batch, out, "column"));
  if (nodes2) {
    RC(fetch(nodes2, 2 * q * batch * 32, out, "nodes"));
    HIP_OK(hipFree(nodes2));
  }
  HIP_OK(hipFree(col));
  HIP_OK(hipFree(vals));
  HIP_OK(hipFree(lo));
  if (hi) HIP_OK(hipFree(hi));
  if (tnodes) HIP_OK(hipFree(tnodes));
  HIP_OK(hipFree(sx));
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s JOBS\n", argv[0]);
    return 2;
  }
  FILE* jf = fopen(argv[1], "r");
  if (!jf) {
    fprintf(stderr, "%s: cannot open\n", argv[1]);
    return 2;
  }
  std::vector<Job> jobs;
  char name[32], inp[4096], outp[4096];
  unsigned long long n, batch, arg;
  int got;
  while ((got = fscanf(jf, "%31s %llu %llu %llu %4095s %4095s", name, &n, &batch, &arg, inp, outp)) == 6) {
    Job j{};
    j.op = 0;
    while (j.op < OP_COUNT && strcmp(OP_NAMES[j.op], name)) ++j.op;
    j.n = n, j.batch = batch, j.arg = arg, j.in = inp, j.out = outp;
    const char* why = j.op == OP_COUNT ? "unknown op" : refuse(j);
    if (why) {
      fprintf(stderr, "bad job %zu (%s %llu %llu %llu): %s\n", jobs.size() + 1, name, n, batch, arg, why);
      fclose(jf);
      return 2;
    }
    jobs.push_back(j);
  }
  fclose(jf);
  if (got != EOF || jobs.empty()) {
    fprintf(stderr, "%s: malformed job line %zu\n", argv[1], jobs.size() + 1);
    return 2;
  }
  for (const Job& j : jobs) {
    std::vector<uint8_t> out;
    const int rc = run_job(j, out);
    if (rc) {
      fprintf(stderr, "job %s %llu %llu %llu failed\n", OP_NAMES[j.op], (unsigned long long)j.n, (unsigned long long)j.batch,
              (unsigned long long)j.arg);
      return rc;
    }
    FILE* f = fopen(j.out.c_str(), "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) {
      fprintf(stderr, "%s: write failed\n", j.out.c_str());
      return 2;
    }
  }
  printf("%zu jobs\n", jobs.size());
  return 0;
}
