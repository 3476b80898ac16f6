// api_modverify.hip -- the verifiers of FRI and STARK proofs over a run-time modulus below 2^256: the host verifiers' entries
// (modverify.hip) and the batch forms (modverify_dev.hip): the plan is checked on the host, then one chain of launches on the ctx stream.
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

int mv_refuse(sh_ctx* c, const char* who, int rc, const char* why) {
  c->err = std::string(who) + ": " + why;
  return rc;
}

// the STARK plan of the shape, or its refusal with the reason in sh_last_error
int mv_stark_plan(sh_ctx* c, MvPlan* p, const uint8_t modulus[32], uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* exps,
                  const uint32_t* counts, uint32_t samples, uint32_t batch, const char* who) {
  const char* why = "";
  const int rc = mv_plan_stark_proof(p, modulus, steps, ext, width, exps, counts, samples, &why);
  if (rc != SH_OK) return mv_refuse(c, who, rc, why);
  if ((uint64_t)p->shape.ys_per_proof * batch > (1ull << 31))  // one lane per sampled row: the grids are 32-bit
    return mv_refuse(c, who, SH_ERR_UNSUPPORTED, "more than 2^31 sampled rows in one call");
  return SH_OK;
}

// upload the terms (skipped when the previous generic call's), then the chain of launches; d_in / d_out: plain limbs
int mv_stark_launch(sh_ctx* c, const MvPlan& p, const void* d_proof, const void* d_in, const void* d_out, uint64_t io_stride,
                    const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts, uint32_t batch, int32_t* d_status) {
  const uint32_t width = p.shape.width;
  uint64_t total = 0;
  for (uint32_t d = 0; d < width; ++d) total += counts[d];
  SH_TRY(mod_stark_terms(c, p.M, width, coefs, exps, counts, total));
  void* ws = nullptr;
  const size_t ys_bytes = mv_round_up((size_t)batch * p.shape.ys_per_proof * 4);
  SH_TRY(ws_get(c, sh_ctx::WS_VB, ys_bytes + (size_t)batch * 4, &ws));
  uint32_t* ys = reinterpret_cast<uint32_t*>(ws);
  uint32_t* flags = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws) + ys_bytes);
  const uint8_t* tb = reinterpret_cast<const uint8_t*>(c->mod_terms_dev);
  HIP_TRY(c, shk_mod_verify_stark_batch(p, static_cast<const uint8_t*>(d_proof), batch, static_cast<const fpm*>(d_in),
                                        static_cast<const fpm*>(d_out), io_stride, reinterpret_cast<const fpm*>(tb + ModTermLayout::coef),
                                        tb + ModTermLayout::exps, width, c->mod_terms_begin, ys, flags, d_status, c->stream));
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

int sh_mod_stark_verify(const uint8_t modulus[32], const uint8_t* proof, uint64_t proof_len, const uint8_t* inputs, const uint8_t* outputs,
                        uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps,
                        const uint32_t* term_counts, uint32_t samples) {
  return mod_stark_verify(modulus, proof, proof_len, inputs, outputs, steps, ext, width, term_coefs, term_exps, term_counts, samples);
}

int sh_dev_mod_stark_verify(sh_ctx* c, const uint8_t modulus[32], const void* d_proof, const void* d_inputs, const void* d_outputs,
                            uint64_t io_stride, uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* term_coefs,
                            const uint8_t* term_exps, const uint32_t* term_counts, uint32_t samples, uint32_t batch, int32_t* d_status) {
  const char* who = "sh_dev_mod_stark_verify";
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !d_proof || !d_inputs || !d_outputs || !d_status || !term_coefs || !term_exps || !term_counts || io_stride == 0 || batch == 0)
    return mv_refuse(c, who, SH_ERR_INVALID, "null pointer, io_stride 0 or batch 0");
  if (((uintptr_t)d_proof | (uintptr_t)d_inputs | (uintptr_t)d_outputs | (uintptr_t)d_status) & 3)  // read as 32-bit words
    return mv_refuse(c, who, SH_ERR_INVALID, "d_proof, d_inputs, d_outputs and d_status must be 4-byte aligned");
  MvPlan p;
  SH_TRY(mv_stark_plan(c, &p, modulus, steps, ext, width, term_exps, term_counts, samples, batch, who));
  SH_TRY(enter(c));
  return mv_stark_launch(c, p, d_proof, d_inputs, d_outputs, io_stride, term_coefs, term_exps, term_counts, batch, d_status);
}

int sh_mod_stark_verify_batch(sh_ctx* c, const uint8_t modulus[32], const uint8_t* proofs, uint64_t proof_len, const uint8_t* inputs,
                              const uint8_t* outputs, uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* term_coefs,
                              const uint8_t* term_exps, const uint32_t* term_counts, uint32_t samples, uint32_t batch, int32_t* status) {
  const char* who = "sh_mod_stark_verify_batch";
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !proofs || !inputs || !outputs || !status || !term_coefs || !term_exps || !term_counts || batch == 0)
    return mv_refuse(c, who, SH_ERR_INVALID, "null pointer, or batch 0");
  MvPlan p;
  SH_TRY(mv_stark_plan(c, &p, modulus, steps, ext, width, term_exps, term_counts, samples, batch, who));
  if (proof_len != p.shape.plen) {  // the host verifier's decision on each mis-sized proof; nothing is launched
    for (uint32_t b = 0; b < batch; ++b)
      status[b] = mod_stark_verify(modulus, proofs + (size_t)b * proof_len, proof_len, inputs + 32ull * width * b, outputs + 32ull * width * b,
                                   steps, ext, width, term_coefs, term_exps, term_counts, samples);
    return mv_refuse(c, who, SH_ERR_INVALID, "proof_len is not sh_stark_proof_len(steps, ext, width, degree, samples)");
  }
  SH_TRY(enter(c));
  // wire form -> limbs is a byte reversal per value; nothing is reduced here (the spot item takes any 256-bit value modulo p)
  const size_t vals = (size_t)batch * width;
  std::vector<uint8_t> limbs(2 * vals * 32);
  for (size_t i = 0; i < 2 * vals; ++i) {
    const uint8_t* src = i < vals ? inputs + 32 * i : outputs + 32 * (i - vals);
    for (int k = 0; k < 32; ++k) limbs[32 * i + k] = src[31 - k];
  }
  const size_t pbytes = mv_round_up((size_t)batch * proof_len), io = mv_round_up(vals * 32);
  void* ws = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_VB_IO, pbytes + 2 * io + (size_t)batch * 4, &ws));
  uint8_t* d = static_cast<uint8_t*>(ws);
  int32_t* d_status = reinterpret_cast<int32_t*>(d + pbytes + 2 * io);
  SH_TRY(h2d(c, d, proofs, (size_t)batch * proof_len));
  SH_TRY(h2d(c, d + pbytes, limbs.data(), vals * 32));
  SH_TRY(h2d(c, d + pbytes + io, limbs.data() + vals * 32, vals * 32));
  SH_TRY(mv_stark_launch(c, p, d, d + pbytes, d + pbytes + io, 1, term_coefs, term_exps, term_counts, batch, d_status));
  return d2h(c, status, d_status, (size_t)batch * 4);
}
}  // extern "C"
