// api_modverify.hip -- the verifiers of FRI proofs over any odd modulus below 2^256: the host verifier's entry (modverify.hip) and the
// batch forms (modverify_dev.hip): the plan is checked on the host, then one chain of launches on the ctx stream.
#include "ctx.hpp"
#include "modverify_items.cuh"
using namespace shk;

namespace {
constexpr size_t MV_ALIGN = 256;
size_t mv_round_up(size_t x) { return (x + MV_ALIGN - 1) & ~(MV_ALIGN - 1); }

// the plan of the shape, or its refusal with the reason in sh_last_error
int mv_plan(sh_ctx* c, MvPlan* p, const uint8_t modulus[32], uint64_t n, const uint8_t root[32], uint64_t md, uint32_t exclude,
            uint32_t samples, const char* who) {
  const char* why = "";
  const int rc = mv_plan_fri_proof(p, modulus, n, root, md, exclude, samples, &why);
  if (rc != SH_OK) {
    c->err = std::string(who) + ": " + why;
    return rc;
  }
  return SH_OK;
}

int mv_launch(sh_ctx* c, const MvPlan& p, const void* d_proof, const void* d_roots, uint32_t batch, int32_t* d_status) {
  if ((uint64_t)p.shape.ys_per_proof * batch > (1ull << 31)) {  // one lane per sampled row: the grids are 32-bit
    c->err = "batch FRI verifier: more than 2^31 sampled rows in one call";
    return SH_ERR_UNSUPPORTED;
  }
  void* ws = nullptr;
  const size_t ys_bytes = mv_round_up((size_t)batch * p.shape.ys_per_proof * 4);
  SH_TRY(ws_get(c, sh_ctx::WS_VB, ys_bytes + (size_t)batch * 4, &ws));
  uint32_t* ys = reinterpret_cast<uint32_t*>(ws);
  uint32_t* flags = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws) + ys_bytes);
  HIP_TRY(c, shk_mod_verify_batch(p, static_cast<const uint8_t*>(d_proof), batch, static_cast<const uint8_t*>(d_roots), ys, flags, d_status,
                                  c->stream));
  return SH_OK;
}
}  // namespace

extern "C" {

int sh_mod_fri_verify(const uint8_t modulus[32], const uint8_t* proof, uint64_t proof_len, const uint8_t merkle_root[32], uint64_t n,
                      const uint8_t root[32], uint64_t maxdeg_plus_1, uint32_t exclude_multiples_of, uint32_t samples) {
  return mod_fri_verify(modulus, proof, proof_len, merkle_root, n, root, maxdeg_plus_1, exclude_multiples_of, samples);
}

int sh_dev_mod_fri_verify(sh_ctx* c, const uint8_t modulus[32], const void* d_proof, const void* d_merkle_roots, uint64_t n,
                          const uint8_t root[32], uint64_t maxdeg_plus_1, uint32_t exclude_multiples_of, uint32_t samples, uint32_t batch,
                          int32_t* d_status) {
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !root || !d_proof || !d_merkle_roots || !d_status || batch == 0) {
    c->err = "sh_dev_mod_fri_verify: null pointer, or batch 0";
    return SH_ERR_INVALID;
  }
  if (((uintptr_t)d_proof | (uintptr_t)d_merkle_roots | (uintptr_t)d_status) & 3) {  // read as 32-bit words
    c->err = "sh_dev_mod_fri_verify: d_proof, d_merkle_roots and d_status must be 4-byte aligned";
    return SH_ERR_INVALID;
  }
  MvPlan p;
  SH_TRY(mv_plan(c, &p, modulus, n, root, maxdeg_plus_1, exclude_multiples_of, samples, "sh_dev_mod_fri_verify"));
  SH_TRY(enter(c));
  return mv_launch(c, p, d_proof, d_merkle_roots, batch, d_status);
}

int sh_mod_fri_verify_batch(sh_ctx* c, const uint8_t modulus[32], const uint8_t* proofs, uint64_t proof_len, const uint8_t* merkle_roots,
                            uint64_t n, const uint8_t root[32], uint64_t maxdeg_plus_1, uint32_t exclude_multiples_of, uint32_t samples,
                            uint32_t batch, int32_t* status) {
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !root || !proofs || !merkle_roots || !status || batch == 0) {
    c->err = "sh_mod_fri_verify_batch: null pointer, or batch 0";
    return SH_ERR_INVALID;
  }
  MvPlan p;
  SH_TRY(mv_plan(c, &p, modulus, n, root, maxdeg_plus_1, exclude_multiples_of, samples, "sh_mod_fri_verify_batch"));
  if (proof_len != p.shape.plen) {  // the host verifier's decision on each mis-sized proof; nothing is launched
    for (uint32_t b = 0; b < batch; ++b)
      status[b] = mod_fri_verify(modulus, proofs + (size_t)b * proof_len, proof_len, merkle_roots + 32ull * b, n, root, maxdeg_plus_1,
                                 exclude_multiples_of, samples);
    c->err = "sh_mod_fri_verify_batch: proof_len is not sh_fri_proof_len(n, maxdeg_plus_1, samples)";
    return SH_ERR_INVALID;
  }
  SH_TRY(enter(c));
  const size_t pbytes = mv_round_up((size_t)batch * proof_len), rbytes = mv_round_up((size_t)batch * 32);
  void* ws = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_VB_IO, pbytes + rbytes + (size_t)batch * 4, &ws));
  uint8_t* d = static_cast<uint8_t*>(ws);
  int32_t* d_status = reinterpret_cast<int32_t*>(d + pbytes + rbytes);
  SH_TRY(h2d(c, d, proofs, (size_t)batch * proof_len));
  SH_TRY(h2d(c, d + pbytes, merkle_roots, (size_t)batch * 32));
  SH_TRY(mv_launch(c, p, d, d + pbytes, batch, d_status));
  return d2h(c, status, d_status, (size_t)batch * 4);
}
}  // extern "C"
