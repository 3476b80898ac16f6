// ctx.hip -- the context of libstarkhip.so: life cycle, workspaces, pinned staging copies, the plan cache, timers and the
// device-memory part of the C ABI declared in include/starkhip.h.
#include "ctx.hpp"
using namespace shk;

namespace {
constexpr size_t PIN_CHUNK = (size_t)8 << 20;

int pin_init(sh_ctx* c) {
  if (c->pin[0]) return SH_OK;
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->pin[i]), PIN_CHUNK, hipHostMallocDefault));
    HIP_TRY(c, hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming));
  }
  return SH_OK;
}
int pin_wait(sh_ctx* c, int slot) {
  if (c->pin_busy[slot]) {
    HIP_TRY(c, hipEventSynchronize(c->pin_ev[slot]));
    c->pin_busy[slot] = false;
  }
  return SH_OK;
}

constexpr size_t MAX_PLANS = 1024;  // count cap of the plan cache (the byte budget normally binds first)

void free_plan(sh_ctx* c, NttPlan* pl) {
  for (void* p : pl->owned) (void)hipFree(p);
  c->plan_bytes -= pl->bytes <= c->plan_bytes ? pl->bytes : c->plan_bytes;
  delete pl;
}

// Free every cached table (NTT plans, the STARK prover's inverse tables) and the workspaces, after the stream drained.
// Everything is rebuilt on demand.
int trim(sh_ctx* c) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (auto& kv : c->plans) free_plan(c, kv.second);
  c->plans.clear();
  c->plan_bytes = 0;
  for (auto& kv : c->inv_z2) (void)hipFree(kv.second);
  c->inv_z2.clear();
  for (auto& kv : c->inv_omega) (void)hipFree(kv.second);
  c->inv_omega.clear();
  for (int i = 0; i < sh_ctx::WS_COUNT; ++i) {
    if (c->ws[i]) (void)hipFree(c->ws[i]);
    c->ws[i] = nullptr;
    c->ws_cap[i] = 0;
  }
  return SH_OK;
}

// Least-recently-used plans go until the cache is inside its byte budget and count cap again; plans looked up recently
// (a prover's hot shapes) stay.  One stream synchronisation if anything is evicted (queued launches may read the tables).
int evict_plans(sh_ctx* c) {
  bool synced = false;
  while (!c->plans.empty() && (c->plan_bytes > c->plan_budget || c->plans.size() + 4 > MAX_PLANS)) {
    auto victim = c->plans.begin();
    for (auto it = c->plans.begin(); it != c->plans.end(); ++it)
      if (it->second->last_use < victim->second->last_use) victim = it;
    if (!synced) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      synced = true;
    }
    free_plan(c, victim->second);
    c->plans.erase(victim);
    ++c->plans_evicted;
  }
  return SH_OK;
}
}  // namespace

namespace shk {
int ws_get(sh_ctx* c, int slot, size_t bytes, void** out) {
  if (bytes == 0) bytes = 32;
  if (bytes > c->ws_cap[slot]) {
    if (c->ws[slot]) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      HIP_TRY(c, hipFree(c->ws[slot]));
      c->ws[slot] = nullptr;
      c->ws_cap[slot] = 0;
    }
    size_t cap = (bytes + 4095) & ~(size_t)4095;
    HIP_TRY(c, hipMalloc(&c->ws[slot], cap));
    c->ws_cap[slot] = cap;
  }
  *out = c->ws[slot];
  return SH_OK;
}

// caller memory the DMA engines can reach directly (sh_host_alloc, hipHostMalloc / hipHostRegister): no staging copy
bool host_is_pinned(const void* h) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, h) != hipSuccess) {
    (void)hipGetLastError();  // an unregistered pointer is an "error" to this query, not to us
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

// host -> device on the ctx stream.  Pageable sources go through the pinned slots (the host memcpy of chunk i+1 overlaps
// the DMA of chunk i) and have been consumed when this returns.  A PINNED source of 64 KiB or more is handed to the DMA
// engine as it is and is read in stream order, i.e. possibly AFTER this returns: the caller must not reuse or free it
// before the stream has passed the copy (every entry point that takes caller buffers synchronises before it returns).
// `staged`: always go through the pinned slots, whatever the size (sources that die right after the call: plan tables).
int h2d(sh_ctx* c, void* d, const void* h, size_t bytes, bool staged) {
  if (bytes == 0) return SH_OK;
  if (!staged && (bytes < ((size_t)64 << 10) || host_is_pinned(h))) {
    HIP_TRY(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    return SH_OK;
  }
  SH_TRY(pin_init(c));
  size_t off = 0;
  for (int i = 0; off < bytes; ++i) {
    const int slot = i & 1;
    const size_t len = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
    SH_TRY(pin_wait(c, slot));
    memcpy(c->pin[slot], static_cast<const uint8_t*>(h) + off, len);
    HIP_TRY(c, hipMemcpyAsync(static_cast<uint8_t*>(d) + off, c->pin[slot], len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->pin_ev[slot], c->stream));
    c->pin_busy[slot] = true;
    off += len;
  }
  return SH_OK;
}
// device -> host (pageable); blocks until `h` is complete.
int d2h(sh_ctx* c, void* h, const void* d, size_t bytes) {
  if (bytes == 0) return SH_OK;
  if (bytes < ((size_t)64 << 10) || host_is_pinned(h)) {
    HIP_TRY(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SH_OK;
  }
  SH_TRY(pin_init(c));
  SH_TRY(pin_wait(c, 0));
  SH_TRY(pin_wait(c, 1));
  size_t off = 0, prev_off = 0, prev_len = 0;
  int prev_slot = -1;
  for (int i = 0; off < bytes; ++i) {
    const int slot = i & 1;
    const size_t len = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
    HIP_TRY(c, hipMemcpyAsync(c->pin[slot], static_cast<const uint8_t*>(d) + off, len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->pin_ev[slot], c->stream));
    if (prev_slot >= 0) {  // drain the previous chunk while this one is in flight
      HIP_TRY(c, hipEventSynchronize(c->pin_ev[prev_slot]));
      memcpy(static_cast<uint8_t*>(h) + prev_off, c->pin[prev_slot], prev_len);
    }
    prev_slot = slot;
    prev_off = off;
    prev_len = len;
    off += len;
  }
  HIP_TRY(c, hipEventSynchronize(c->pin_ev[prev_slot]));
  memcpy(static_cast<uint8_t*>(h) + prev_off, c->pin[prev_slot], prev_len);
  return SH_OK;
}

// ---- the plan cache (ctx.hpp) ---------------------------------------------------------------------------
// device allocation owned by (and accounted to) a plan
int plan_alloc(sh_ctx* c, NttPlan* pl, size_t bytes, void** out) {
  void* d = nullptr;
  HIP_TRY(c, hipMalloc(&d, bytes ? bytes : 32));
  pl->owned.push_back(d);
  pl->bytes += bytes;
  *out = d;
  return SH_OK;
}
NttPlan* plan_find(sh_ctx* c, const std::string& key) {
  auto it = c->plans.find(key);
  if (it == c->plans.end()) return nullptr;
  it->second->last_use = ++c->tick;
  return it->second;
}
PlanHolder::~PlanHolder() {
  if (!p) return;
  for (void* d : p->owned) (void)hipFree(d);
  delete p;
}
NttPlan* plan_commit(sh_ctx* c, const std::string& key, PlanHolder* h) {
  NttPlan* pl = h->p;
  h->p = nullptr;
  pl->last_use = ++c->tick;
  c->plan_bytes += pl->bytes;
  ++c->plans_built;
  c->plans[key] = pl;
  return pl;
}

// Called on entry of every public function that builds plans, never while a plan pointer is held: a long-lived prover
// that meets many shapes must not grow for ever (a call creates at most 4 plans, so the budget can be overshot by one
// call's tables until the next entry).
int enter(sh_ctx* c) {
  HIP_TRY(c, hipSetDevice(c->device));
  return evict_plans(c);
}

// ---- host-buffer API: wire-form uploads and downloads ------------------------------------------------
int upload_padded(sh_ctx* c, const uint8_t* in, uint64_t n_in, uint64_t n, uint32_t batch, int slot, fp** out) {
  void *w = nullptr, *x = nullptr, *y = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)batch * (n_in > n ? n_in : n) * 32, &w));
  SH_TRY(ws_get(c, slot, (size_t)batch * n * sizeof(fp), &x));
  if (n_in == n) {
    SH_TRY(h2d(c, w, in, (size_t)batch * n * 32));
    HIP_TRY(c, shk_wire_to_limb(reinterpret_cast<uint8_t*>(w), reinterpret_cast<fp*>(x), (uint64_t)batch * n, c->stream));
  } else {
    SH_TRY(ws_get(c, sh_ctx::WS_MISC, (size_t)batch * (n_in ? n_in : 1) * sizeof(fp), &y));
    if (n_in) {
      SH_TRY(h2d(c, w, in, (size_t)batch * n_in * 32));
      HIP_TRY(c, shk_wire_to_limb(reinterpret_cast<uint8_t*>(w), reinterpret_cast<fp*>(y), (uint64_t)batch * n_in, c->stream));
    }
    HIP_TRY(c, shk_pad_copy(reinterpret_cast<fp*>(y), reinterpret_cast<fp*>(x), n_in, n, batch, c->stream));  // fft.py:323-324
  }
  *out = reinterpret_cast<fp*>(x);
  return SH_OK;
}
// 0 < n_in < n: the values as they are ([batch][n_in] in WS_Y, a slot no FRI / NTT driver touches); the transform's first pass takes the zero padding as
// implicit (run_ntt's n_in).  Otherwise the padded array of upload_padded, *n_short = 0.
int upload_short(sh_ctx* c, const uint8_t* in, uint64_t n_in, uint64_t n, uint32_t batch, int slot, fp** out,
                        uint64_t* n_short) {
  *n_short = 0;
  if (n_in == 0 || n_in >= n) return upload_padded(c, in, n_in, n, batch, slot, out);
  void *w = nullptr, *y = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)batch * n * 32, &w));  // sized for the n-point result's download as well
  SH_TRY(ws_get(c, sh_ctx::WS_Y, (size_t)batch * n_in * sizeof(fp), &y));
  SH_TRY(h2d(c, w, in, (size_t)batch * n_in * 32));
  HIP_TRY(c, shk_wire_to_limb(reinterpret_cast<uint8_t*>(w), reinterpret_cast<fp*>(y), (uint64_t)batch * n_in, c->stream));
  *out = reinterpret_cast<fp*>(y);
  *n_short = n_in;
  return SH_OK;
}
int download_wire(sh_ctx* c, const fp* d, uint8_t* out, uint64_t count) {
  void* w = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)count * 32, &w));
  HIP_TRY(c, shk_limb_to_wire(d, reinterpret_cast<uint8_t*>(w), count, c->stream));
  return d2h(c, out, w, (size_t)count * 32);
}
}  // namespace shk

extern "C" {

const char* sh_strerror(int status) {
  switch (status) {
    case SH_OK: return "ok";
    case SH_ERR_INVALID: return "invalid argument";
    case SH_ERR_ROOT_ORDER: return "root_of_unity does not have order n";
    case SH_ERR_HIP: return "HIP runtime error";
    case SH_ERR_NOMEM: return "out of memory";
    case SH_ERR_TOO_SMALL: return "output buffer too small";
    case SH_ERR_UNSUPPORTED: return "unsupported size";
    case SH_ERR_CONSTRAINT: return "the witness violates a transition constraint";
    case SH_ERR_NO_DEVICE: return "no usable gfx950 device";
    case SH_ERR_REJECTED: return "proof rejected";
    default: return "unknown status";
  }
}
const char* sh_version(void) { return "starkhip 0.1 (gfx950)"; }

int sh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sh_ctx_create(int device, sh_ctx** out) {
  if (!out) return SH_ERR_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return SH_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SH_ERR_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SH_ERR_NO_DEVICE;  // the code objects are gfx950 only
  sh_ctx* c = new sh_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return SH_ERR_HIP;
  }
  if (shk_knobs().plan_cache_mb >= 0) c->plan_budget = (size_t)shk_knobs().plan_cache_mb << 20;
  *out = c;
  return SH_OK;
}

void sh_ctx_destroy(sh_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)trim(c);
  if (c->terms_dev) (void)hipFree(c->terms_dev);
  if (c->mod_terms_dev) (void)hipFree(c->mod_terms_dev);
  if (c->mod64_terms_dev) (void)hipFree(c->mod64_terms_dev);
  if (c->bad_flag) (void)hipFree(c->bad_flag);
  for (int i = 0; i < 2; ++i) {
    if (c->pin[i]) (void)hipHostFree(c->pin[i]);
    if (c->pin_ev[i]) (void)hipEventDestroy(c->pin_ev[i]);
  }
  (void)hipEventDestroy(c->ev0);
  (void)hipEventDestroy(c->ev1);
  if (c->io_in) (void)hipStreamSynchronize(c->io_in);
  if (c->io_out) (void)hipStreamSynchronize(c->io_out);
  if (c->io_ev) (void)hipEventDestroy(c->io_ev);
  if (c->io_in) (void)hipStreamDestroy(c->io_in);
  if (c->io_out) (void)hipStreamDestroy(c->io_out);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* sh_last_error(const sh_ctx* c) { return c ? c->err.c_str() : ""; }

int sh_sync(sh_ctx* c) {
  if (!c) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}
int sh_timer_start(sh_ctx* c) {
  if (!c) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  return SH_OK;
}
int sh_timer_stop(sh_ctx* c, float* ms) {
  if (!c || !ms) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  HIP_TRY(c, hipEventSynchronize(c->ev1));
  HIP_TRY(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
  return SH_OK;
}

// ---- device-resident API ------------------------------------------------------------------------------
int sh_dev_alloc(sh_ctx* c, uint64_t bytes, void** dptr) {
  if (!c || !dptr) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMalloc(dptr, bytes ? bytes : 32));
  return SH_OK;
}
int sh_dev_free(sh_ctx* c, void* dptr) {
  if (!c) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipFree(dptr));
  return SH_OK;
}
int sh_dev_upload(sh_ctx* c, const void* host_src, void* d_dst, uint64_t bytes) {
  if (!c || (!host_src && bytes) || (!d_dst && bytes)) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  SH_TRY(h2d(c, d_dst, host_src, bytes));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}
int sh_dev_download(sh_ctx* c, const void* d_src, void* host_dst, uint64_t bytes) {
  if (!c || (!host_dst && bytes) || (!d_src && bytes)) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  return d2h(c, host_dst, d_src, bytes);
}
int sh_host_alloc(sh_ctx* c, uint64_t bytes, void** hptr) {
  if (!c || !hptr) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipHostMalloc(hptr, bytes ? bytes : 32, hipHostMallocDefault));
  return SH_OK;
}
int sh_host_free(sh_ctx* c, void* hptr) {
  if (!c) {
    // the context that allocated it is gone (sh_ctx_destroy frees no caller buffers): a pinned buffer belongs to the process,
    // so it can still be released -- device-wide, since no stream is left to drain
    if (!hptr) return SH_OK;
    if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
    return hipHostFree(hptr) == hipSuccess ? SH_OK : SH_ERR_HIP;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipHostFree(hptr));
  return SH_OK;
}
int sh_dev_download_async(sh_ctx* c, const void* d_src, void* host_dst, uint64_t bytes) {
  if (!c || (bytes && (!d_src || !host_dst))) return SH_ERR_INVALID;
  if (!bytes) return SH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!host_is_pinned(host_dst)) return SH_ERR_INVALID;  // a pageable destination would make the copy synchronous and staged
  if (!c->io_out) HIP_TRY(c, hipStreamCreateWithFlags(&c->io_out, hipStreamNonBlocking));
  if (!c->io_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->io_ev, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(c->io_ev, c->stream));           // behind the work queued so far ...
  HIP_TRY(c, hipStreamWaitEvent(c->io_out, c->io_ev, 0));    // ... (the wait is enqueued, the event may be re-recorded at once)
  HIP_TRY(c, hipMemcpyAsync(host_dst, d_src, bytes, hipMemcpyDeviceToHost, c->io_out));
  return SH_OK;
}
int sh_io_sync(sh_ctx* c) {
  if (!c) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->io_in) HIP_TRY(c, hipStreamSynchronize(c->io_in));
  if (c->io_out) HIP_TRY(c, hipStreamSynchronize(c->io_out));
  return SH_OK;
}
int sh_dev_copy(sh_ctx* c, const void* d_src, void* d_dst, uint64_t bytes) {
  if (!c || (bytes && (!d_src || !d_dst))) return SH_ERR_INVALID;
  if (!bytes) return SH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, c->stream));
  return SH_OK;
}
int sh_dev_download_2d(sh_ctx* c, const void* d_src, uint64_t src_pitch, void* host_dst, uint64_t width, uint64_t rows) {
  if (!c || !d_src || !host_dst || width > src_pitch) return SH_ERR_INVALID;
  if (!width || !rows) return SH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy2DAsync(host_dst, width, d_src, src_pitch, width, rows, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}
int sh_dev_from_wire(sh_ctx* c, const uint8_t* host_wire, void* d_limbs, uint64_t n) {
  if (!c || (n && (!host_wire || !d_limbs))) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  void* w = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, n * 32, &w));
  SH_TRY(h2d(c, w, host_wire, n * 32));
  HIP_TRY(c, shk_wire_to_limb(reinterpret_cast<const uint8_t*>(w), reinterpret_cast<fp*>(d_limbs), n, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}
int sh_dev_to_wire(sh_ctx* c, const void* d_limbs, uint8_t* host_wire, uint64_t n) {
  if (!c || (n && (!host_wire || !d_limbs))) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  void* w = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, n * 32, &w));
  HIP_TRY(c, shk_limb_to_wire(reinterpret_cast<const fp*>(d_limbs), reinterpret_cast<uint8_t*>(w), n, c->stream));
  return d2h(c, host_wire, w, n * 32);
}
int sh_dev_fill_seeded(sh_ctx* c, void* d_limbs, uint64_t n, uint64_t seed) {
  if (!c || (n && !d_limbs)) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, shk_fill_seeded(reinterpret_cast<fp*>(d_limbs), n, seed, c->stream));
  return SH_OK;
}
int sh_ctx_trim(sh_ctx* c) {
  if (!c) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  return trim(c);
}
int sh_ctx_set_plan_budget(sh_ctx* c, uint64_t bytes) {
  if (!c) return SH_ERR_INVALID;
  c->plan_budget = (size_t)bytes;
  return enter(c);
}
int sh_ctx_stats(const sh_ctx* c, uint64_t out[4]) {
  if (!c || !out) return SH_ERR_INVALID;
  out[0] = c->plans.size();
  out[1] = c->plan_bytes;
  out[2] = c->plans_built;
  out[3] = c->plans_evicted;
  return SH_OK;
}
}  // extern "C"
