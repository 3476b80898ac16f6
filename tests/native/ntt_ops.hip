// Every NTT pass kernel of starks_amd/csrc/ntt.hip on its own, one named instantiation per job (shk_launch_ntt_cell), and the small
// kernels around the passes: the harness of tests/test_ntt_passes_host.py (cross-compile, refusals) and tests/test_gpu_ntt_passes.py
// (every case of tests/ntt_cases.py on the device).  Built with ntt.hip and kernels.hip alone:
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -I starks_amd/csrc ntt_ops.hip ntt.hip kernels.hip
//   ntt_ops JOBS    JOBS: one job per line, "op key=value ..."; every line is checked before the first HIP call.
// Values in `in` are 32-byte wire elements (big-endian, possibly >= p), loaded through shk_wire_to_limb, so an unreduced value
// stays unreduced on the device.  The harness does NO field arithmetic: every table comes from `in`, in this order:
//   pass    wR [n_wr][2] (each entry, then its canonical image times 2^128), tw2 [n_tw2], lo [n_lo], hi [n_hi], scale [scale], src [n_src]
//           keys: log_R last form (0 tile, 1 narrow) tile_log xcd total log_n log_S log_P tw (0 none, 1 tw2, 2 direct lo, 3 lo * hi) lb
//                 ndig d0 d1 d2 scale src_n pass_index inplace n_wr n_tw2 n_lo n_hi n_src
//           out: dst, total * R elements (src_n: whole vectors of n)          -- shk_launch_ntt_cell, every NttPassArgs field from the job
//   tiny    scale [scale], src [n_src]; keys n batch scale n_src; out [batch][n]   -- shk_launch_ntt_tiny
//   tw2     lo [n_lo], hi [n_hi]; keys log_R log_S lb n_lo n_hi; out [R][S]          -- shk_tw2
//   powers  lo [n_lo], hi [n_hi]; keys n lb n_lo n_hi; out [n]                      -- shk_powers
//   pad     src [batch][n_in]; keys n n_in batch; out [batch][n]                    -- shk_pad_copy
// A source of n_src elements (whole vectors) shorter than the job needs is repeated cyclically: large batches from small files.
// Outputs are the limbs the kernel stored (32 bytes per element, little-endian words), any representative in [0, 2^256).
// Every output buffer starts as 0xa5 bytes (inplace: as the source) and runs GUARD bytes past its end; a guard byte that changed
// ends the run with status 4.  Status 2: a job the harness refuses -- a table shorter than the largest index the kernel can read,
// a source that does not cover its vectors, inconsistent sizes, a cell that does not exist, too many elements -- nothing is run
// and nothing written; 3: a HIP error.  No job can make a kernel read or write outside its buffers.
// Each job prints "name chosen=form/tile_log/xcd": for a pass, the cell shk_ntt_choose_cell gives those arguments under the
// environment of the process (the job itself runs in the cell it names).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <map>
#include <string>
#include <vector>

#include "internal.hpp"

constexpr size_t GUARD = 4096;
constexpr uint64_t MAX_ELEMS = 1ull << 22;  // elements per buffer
constexpr uint32_t MAX_LOG_N = 26;

struct Job {
  std::string op, name, in, out;
  std::map<std::string, uint64_t> k;
  uint64_t get(const char* key) const {
    auto it = k.find(key);
    return it == k.end() ? 0 : it->second;
  }
  // derived by refuse()
  uint64_t out_elems = 0, src_need = 0, src_vec = 0;
};

static const char* const PASS_KEYS[] = {"log_R", "last", "form", "tile_log", "xcd", "total", "log_n", "log_S", "log_P", "tw", "lb", "ndig",
                                        "d0", "d1", "d2", "scale", "src_n", "pass_index", "inplace", "n_wr", "n_tw2", "n_lo", "n_hi",
                                        "n_src", nullptr};
static const char* const TINY_KEYS[] = {"n", "batch", "scale", "n_src", nullptr};
static const char* const TW2_KEYS[] = {"log_R", "log_S", "lb", "n_lo", "n_hi", nullptr};
static const char* const POWERS_KEYS[] = {"n", "lb", "n_lo", "n_hi", nullptr};
static const char* const PAD_KEYS[] = {"n", "n_in", "batch", nullptr};

static const char* const* keys_of(const std::string& op) {
  return op == "pass" ? PASS_KEYS : op == "tiny" ? TINY_KEYS : op == "tw2" ? TW2_KEYS : op == "powers" ? POWERS_KEYS : op == "pad" ? PAD_KEYS : nullptr;
}

static long long file_size(const char* path) {
  struct stat st;
  return stat(path, &st) == 0 ? (long long)st.st_size : -1;
}

// lo / hi must cover every exponent e <= emax: lo[e] (no hi), or lo[e & mask] and hi[e >> lb]
static const char* table_short(uint64_t emax, bool has_hi, uint64_t lb, uint64_t n_lo, uint64_t n_hi) {
  if (!has_hi) return n_lo < emax + 1 ? "lo does not cover the largest exponent" : nullptr;
  if (lb > 30) return "lb must be at most 30";
  const uint64_t mask = (1ull << lb) - 1;
  if (n_lo < (emax < mask ? emax : mask) + 1) return "lo does not cover e & mask";
  if (n_hi < (emax >> lb) + 1) return "hi does not cover e >> lb";
  return nullptr;
}

static const char* refuse(Job& j) {
  const long long sz = file_size(j.in.c_str());
  if (sz < 0) return "cannot read the input";
  uint64_t file_elems = 0;
  if (j.op == "pass") {
    const uint64_t log_R = j.get("log_R"), last = j.get("last"), form = j.get("form"), tile_log = j.get("tile_log"), xcd = j.get("xcd");
    const uint64_t total = j.get("total"), log_n = j.get("log_n"), log_S = j.get("log_S"), log_P = j.get("log_P"), tw = j.get("tw");
    const uint64_t ndig = j.get("ndig"), scale = j.get("scale"), src_n = j.get("src_n"), inplace = j.get("inplace");
    const uint64_t n_wr = j.get("n_wr"), n_tw2 = j.get("n_tw2"), n_lo = j.get("n_lo"), n_hi = j.get("n_hi"), n_src = j.get("n_src");
    if (last > 1 || xcd > 1 || scale > 1 || inplace > 1 || form > 1 || tile_log > 12) return "a flag is out of range";
    if (!shk_ntt_cell_exists((int)form, (int)tile_log, (int)log_R)) return "no such cell";
    if (xcd && form != SHK_NTT_TILE) return "only tile launches take the XCD mapping";
    if (log_n > MAX_LOG_N || log_S > MAX_LOG_N || log_P > MAX_LOG_N || log_R > log_n) return "sizes out of range";
    if (total == 0 || total > MAX_ELEMS) return "total must be 1 .. the element cap";
    if (j.get("pass_index") > 0xffffffffull) return "pass_index out of range";
    const uint64_t R = 1ull << log_R, n = 1ull << log_n, elems = total << log_R;
    if (elems > MAX_ELEMS) return "too many elements";
    if (elems % n) return "total is not a whole number of vectors";
    if (n_wr < R / 2) return "wR needs R/2 pairs";
    if (n_wr > MAX_ELEMS || n_tw2 > MAX_ELEMS || n_lo > MAX_ELEMS || n_hi > MAX_ELEMS || n_src > MAX_ELEMS) return "a table is too long";
    if (last) {
      if (log_P + log_R != log_n || log_S) return "a row pass has P = n / R rows per vector and no log_S";
      if (tw || n_tw2 || n_lo || n_hi || j.get("lb")) return "a row pass has no inter-pass twiddles";
      if (ndig > 3) return "ndig must be 0 .. 3";
      uint64_t sum = 0;
      const uint64_t d[3] = {j.get("d0"), j.get("d1"), j.get("d2")};
      for (uint64_t i = 0; i < 3; ++i) {
        if (i < ndig ? (d[i] < 1 || d[i] > MAX_LOG_N) : d[i] != 0) return "digit widths must be >= 1, unused ones 0";
        sum += d[i];
      }
      if (sum != log_P) return "digit widths must sum to log_P";
      if ((src_n || inplace) && log_P) return "src_n and inplace need the single-pass form (P = 1)";
    } else {
      if (log_P || ndig || j.get("d0") || j.get("d1") || j.get("d2") || scale) return "a column pass has no digits, log_P or scale";
      if (log_R + log_S > log_n) return "R * S exceeds n";
      if (total & ((1ull << log_S) - 1)) return "total is not a whole number of column blocks";
      const uint64_t S = 1ull << log_S, emax = (S - 1) * (R - 1);
      if (tw == 1) {
        if (n_tw2 < R * S) return "tw2 needs R * S entries";
        if (n_lo || n_hi || j.get("lb")) return "tw2 jobs carry no lo / hi";
      } else if (tw == 2 || tw == 3) {
        if (n_tw2) return "lo / hi jobs carry no tw2";
        if (tw == 2 && (n_hi || j.get("lb"))) return "a direct table has no hi";
        if (const char* why = table_short(emax, tw == 3, j.get("lb"), n_lo, n_hi)) return why;
      } else {
        return "a column pass needs tw = 1, 2 or 3";
      }
      if (src_n && log_R + log_S != log_n) return "src_n needs the first pass (P = 1)";
    }
    if (src_n > n) return "src_n exceeds n";
    if (src_n && inplace) return "a short source cannot alias the destination";
    j.src_vec = src_n ? src_n : n;
    j.src_need = (elems / n) * j.src_vec;
    j.out_elems = elems;
    if (n_src < j.src_vec || n_src % j.src_vec || n_src > j.src_need) return "the source must hold whole vectors (src_n or n elements each), at most the batch";
    file_elems = 2 * n_wr + n_tw2 + n_lo + n_hi + scale + n_src;
  } else if (j.op == "tiny") {
    const uint64_t n = j.get("n"), batch = j.get("batch"), n_src = j.get("n_src");
    if (n != 1 && n != 2) return "n must be 1 or 2";
    if (j.get("scale") > 1) return "scale must be 0 or 1";
    if (batch == 0 || batch > MAX_ELEMS / 2) return "batch out of range";
    j.src_vec = n, j.src_need = n * batch, j.out_elems = n * batch;
    if (n_src < n || n_src % n || n_src > j.src_need) return "the source must hold whole vectors, at most the batch";
    file_elems = j.get("scale") + n_src;
  } else if (j.op == "tw2" || j.op == "powers") {
    const uint64_t lb = j.get("lb"), n_lo = j.get("n_lo"), n_hi = j.get("n_hi");
    uint64_t n;
    if (j.op == "tw2") {
      if (j.get("log_R") > MAX_LOG_N || j.get("log_S") > MAX_LOG_N || j.get("log_R") + j.get("log_S") > 22) return "R * S too large";
      n = 1ull << (j.get("log_R") + j.get("log_S"));
    } else {
      n = j.get("n");
      if (n == 0 || n > MAX_ELEMS) return "n out of range";
    }
    if (n_lo > MAX_ELEMS || n_hi > MAX_ELEMS || n_lo == 0) return "table length out of range";
    if (n_hi == 0 && j.op == "powers") {
      // powers without hi reads lo[i & mask]
      if (lb > 30) return "lb must be at most 30";
      const uint64_t mask = (1ull << lb) - 1;
      if (n_lo < ((n - 1) < mask ? (n - 1) : mask) + 1) return "lo does not cover i & mask";
    } else if (const char* why = table_short(n - 1, n_hi != 0, lb, n_lo, n_hi)) {
      return why;
    }
    j.out_elems = n;
    file_elems = n_lo + n_hi;
  } else if (j.op == "pad") {
    const uint64_t n = j.get("n"), n_in = j.get("n_in"), batch = j.get("batch");
    if (n == 0 || batch == 0 || n > MAX_ELEMS || batch > MAX_ELEMS || n * batch > MAX_ELEMS) return "n * batch out of range";
    if (n_in > n) return "n_in exceeds n";
    j.out_elems = n * batch;
    file_elems = n_in * batch;
  } else {
    return "unknown op";
  }
  if ((uint64_t)sz != 32 * file_elems) return "input size does not match the job";
  return nullptr;
}

#define HIP_OK(x)                                             \
  do {                                                        \
    const hipError_t e_ = (x);                                \
    if (e_ != hipSuccess) {                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      return 3;                                               \
    }                                                         \
  } while (0)
#define RC(x)           \
  do {                  \
    const int r_ = (x); \
    if (r_) return r_;  \
  } while (0)

static bool read_file(const char* path, std::vector<uint8_t>& v) {
  const long long sz = file_size(path);
  FILE* f = fopen(path, "rb");
  if (!f || sz < 0) return false;
  v.resize((size_t)sz);
  const bool ok = fread(v.data(), 1, v.size(), f) == v.size();
  fclose(f);
  return ok;
}

// `n` wire values -> `want` >= n limb elements on the device (the n values repeated cyclically), followed by `guard` bytes of 0xa5
static int to_limbs(const uint8_t* wire, uint64_t n, uint64_t want, size_t guard, fp** d) {
  uint8_t* w = nullptr;
  HIP_OK(hipMalloc((void**)&w, n ? 32 * n : 32));
  if (n) HIP_OK(hipMemcpy(w, wire, 32 * n, hipMemcpyHostToDevice));
  if (want < n) want = n;
  HIP_OK(hipMalloc((void**)d, 32 * (want ? want : 1) + guard));
  if (guard) HIP_OK(hipMemset(reinterpret_cast<uint8_t*>(*d) + 32 * want, 0xa5, guard));
  HIP_OK(shk_wire_to_limb(w, *d, n, 0));
  HIP_OK(hipDeviceSynchronize());
  for (uint64_t at = n; n && at < want; at += n)
    HIP_OK(hipMemcpy(*d + at, *d, 32 * (want - at < n ? want - at : n), hipMemcpyDeviceToDevice));
  HIP_OK(hipFree(w));
  return 0;
}
static int alloc_out(uint64_t elems, fp** d) {
  HIP_OK(hipMalloc((void**)d, 32 * elems + GUARD));
  HIP_OK(hipMemset(*d, 0xa5, 32 * elems + GUARD));
  return 0;
}
static int fetch(const fp* d, uint64_t elems, std::vector<uint8_t>& out) {
  out.resize(32 * elems + GUARD);
  HIP_OK(hipMemcpy(out.data(), d, out.size(), hipMemcpyDeviceToHost));
  for (size_t i = 32 * elems; i < out.size(); ++i)
    if (out[i] != 0xa5) {
      fprintf(stderr, "guard byte %zu past the end (%llu elements) was written\n", i - 32 * elems, (unsigned long long)elems);
      return 4;
    }
  out.resize(32 * elems);
  return 0;
}

static int run_job(const Job& j, std::vector<uint8_t>& out) {
  std::vector<uint8_t> in;
  if (!read_file(j.in.c_str(), in)) {
    fprintf(stderr, "%s: cannot read\n", j.in.c_str());
    return 2;
  }
  const uint8_t* p = in.data();
  std::vector<fp*> owned;
  auto table = [&](uint64_t n, fp** d) {
    *d = nullptr;
    if (!n) return 0;
    const int rc = to_limbs(p, n, n, 0, d);
    p += 32 * n;
    owned.push_back(*d);
    return rc;
  };
  fp* dst = nullptr;
  if (j.op == "pass") {
    fp *wr, *tw2, *lo, *hi, *scale, *src;
    RC(table(2 * j.get("n_wr"), &wr));
    RC(table(j.get("n_tw2"), &tw2));
    RC(table(j.get("n_lo"), &lo));
    RC(table(j.get("n_hi"), &hi));
    RC(table(j.get("scale"), &scale));
    const bool inplace = j.get("inplace");
    RC(to_limbs(p, j.get("n_src"), j.src_need, inplace ? GUARD : 0, &src));
    owned.push_back(src);
    if (inplace) dst = src;
    else RC(alloc_out(j.out_elems, &dst));
    NttPassArgs a;
    memset(&a, 0, sizeof a);
    a.src = src, a.dst = dst, a.total = j.get("total");
    a.log_n = (uint32_t)j.get("log_n"), a.log_S = (uint32_t)j.get("log_S"), a.log_P = (uint32_t)j.get("log_P");
    a.wR = reinterpret_cast<const fp2*>(wr);
    a.tw_lo = lo, a.tw_hi = hi, a.tw_lb = (uint32_t)j.get("lb"), a.tw_direct = j.get("tw") == 2;
    a.ndig = (uint32_t)j.get("ndig");
    a.dig_log[0] = (uint32_t)j.get("d0"), a.dig_log[1] = (uint32_t)j.get("d1"), a.dig_log[2] = (uint32_t)j.get("d2");
    a.scale = scale, a.src_n = j.get("src_n"), a.tw2 = tw2, a.pass_index = (uint32_t)j.get("pass_index");
    const ShkNttCell cell{(int)j.get("form"), (int)j.get("tile_log"), j.get("xcd") != 0};
    HIP_OK(shk_launch_ntt_cell(cell, (int)j.get("log_R"), j.get("last") != 0, a, 0));
  } else if (j.op == "tiny") {
    fp *scale, *src;
    RC(table(j.get("scale"), &scale));
    RC(to_limbs(p, j.get("n_src"), j.src_need, 0, &src));
    owned.push_back(src);
    RC(alloc_out(j.out_elems, &dst));
    HIP_OK(shk_launch_ntt_tiny(src, dst, (uint32_t)j.get("n"), (uint32_t)j.get("batch"), scale, 0));
  } else if (j.op == "tw2" || j.op == "powers") {
    fp *lo, *hi;
    RC(table(j.get("n_lo"), &lo));
    RC(table(j.get("n_hi"), &hi));
    RC(alloc_out(j.out_elems, &dst));
    if (j.op == "tw2") HIP_OK(shk_tw2(lo, hi, (uint32_t)j.get("lb"), dst, (uint32_t)j.get("log_R"), (uint32_t)j.get("log_S"), 0));
    else HIP_OK(shk_powers(lo, hi, (uint32_t)j.get("lb"), dst, j.get("n"), 0));
  } else {
    fp* src;
    RC(to_limbs(p, j.get("n_in") * j.get("batch"), 0, 0, &src));
    owned.push_back(src);
    RC(alloc_out(j.out_elems, &dst));
    HIP_OK(shk_pad_copy(src, dst, j.get("n_in"), j.get("n"), (uint32_t)j.get("batch"), 0));
  }
  HIP_OK(hipDeviceSynchronize());
  RC(fetch(dst, j.out_elems, out));
  bool dst_owned = false;
  for (fp* d : owned) {
    dst_owned |= d == dst;
    HIP_OK(hipFree(d));
  }
  if (!dst_owned) HIP_OK(hipFree(dst));
  return 0;
}

static bool parse_line(char* line, Job& j, std::string& why) {
  char* save = nullptr;
  char* tok = strtok_r(line, " \t\r\n", &save);
  if (!tok) return false;
  j.op = tok;
  const char* const* keys = keys_of(j.op);
  if (!keys) {
    why = "unknown op";
    return true;
  }
  while ((tok = strtok_r(nullptr, " \t\r\n", &save))) {
    char* eq = strchr(tok, '=');
    if (!eq || eq == tok || !eq[1]) {
      why = "malformed token";
      return true;
    }
    const std::string key(tok, eq - tok), val(eq + 1);
    if (key == "in") j.in = val;
    else if (key == "out") j.out = val;
    else if (key == "name") j.name = val;
    else {
      bool known = false;
      for (const char* const* q = keys; *q; ++q) known |= key == *q;
      char* end = nullptr;
      const unsigned long long v = strtoull(val.c_str(), &end, 10);
      if (!known || *end || val[0] == '-' || j.k.count(key)) {
        why = "unknown, repeated or non-numeric key " + key;
        return true;
      }
      j.k[key] = v;
    }
  }
  if (j.in.empty() || j.out.empty()) why = "in= and out= are required";
  else
    for (const char* const* q = keys; *q; ++q)
      if (!j.k.count(*q)) why = std::string("missing key ") + *q;
  return true;
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
  static char line[16384];
  while (fgets(line, sizeof line, jf)) {
    Job j;
    std::string why;
    const std::string copy(line);
    if (!parse_line(line, j, why)) continue;  // an empty line
    if (why.empty())
      if (const char* w = refuse(j)) why = w;
    if (!why.empty()) {
      fprintf(stderr, "bad job %zu (%s): %s\n", jobs.size() + 1, copy.c_str(), why.c_str());
      fclose(jf);
      return 2;
    }
    jobs.push_back(j);
  }
  fclose(jf);
  if (jobs.empty()) {
    fprintf(stderr, "%s: no jobs\n", argv[1]);
    return 2;
  }
  for (const Job& j : jobs) {
    std::vector<uint8_t> out;
    const int rc = run_job(j, out);
    if (rc) {
      fprintf(stderr, "job %s %s failed\n", j.op.c_str(), j.name.c_str());
      return rc;
    }
    FILE* f = fopen(j.out.c_str(), "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) {
      fprintf(stderr, "%s: write failed\n", j.out.c_str());
      return 2;
    }
    if (j.op == "pass") {
      const ShkNttPassShape shape{j.get("total"), (unsigned)j.get("log_n"), (unsigned)j.get("log_S"), (unsigned)j.get("pass_index")};
      const ShkNttCell c = shk_ntt_choose_cell(shk_knobs(), (int)j.get("log_R"), j.get("last") != 0, shape);
      printf("%s chosen=%d/%d/%d\n", j.name.c_str(), c.form, c.tile_log, (int)c.xcd);
    } else {
      printf("%s chosen=-\n", j.name.c_str());
    }
    fflush(stdout);
  }
  printf("%zu jobs\n", jobs.size());
  return 0;
}
