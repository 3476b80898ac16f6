// api_verify.hip -- the batch verifiers (verify_dev.hip): the plan is checked on the host, then one chain of launches on the ctx stream.
#include "ctx.hpp"
using namespace shk;

namespace {
constexpr size_t VB_ALIGN = 256;
size_t vb_round_up(size_t x) { return (x + VB_ALIGN - 1) & ~(VB_ALIGN - 1); }

int vb_launch(sh_ctx* c, const VbPlan& p, const void* d_proof, const void* d_roots, const void* d_in, const void* d_out,
              uint64_t io_stride, uint32_t batch, int32_t* d_status) {
  void* ws = nullptr;
  const size_t ys_bytes = vb_round_up((size_t)batch * p.ys_per_proof * 4);
  SH_TRY(ws_get(c, sh_ctx::WS_VB, ys_bytes + (size_t)batch * 4, &ws));
  uint32_t* ys = reinterpret_cast<uint32_t*>(ws);
  uint32_t* flags = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws) + ys_bytes);
  const uint8_t* tb = reinterpret_cast<const uint8_t*>(c->terms_dev);
  HIP_TRY(c, shk_verify_batch(p, static_cast<const uint8_t*>(d_proof), batch, static_cast<const uint8_t*>(d_roots),
                              static_cast<const fp*>(d_in), static_cast<const fp*>(d_out), io_stride,
                              p.stark ? reinterpret_cast<const fp*>(tb + TermLayout::coef) : nullptr,
                              p.stark ? tb + TermLayout::exps : nullptr, p.width + 1, c->terms_begin, ys, flags, d_status, c->stream));
  return SH_OK;
}
}  // namespace

extern "C" {

int sh_dev_stark_verify(sh_ctx* c, const void* d_proof, const void* d_inputs, const void* d_outputs, uint64_t io_stride, uint64_t steps,
                        uint32_t ext, uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts,
                        uint32_t samples, uint32_t batch, int32_t* d_status) {
  if (!c || !d_proof || !d_inputs || !d_outputs || !d_status || !term_coefs || io_stride == 0 || batch == 0) return SH_ERR_INVALID;
  if (((uintptr_t)d_proof | (uintptr_t)d_inputs | (uintptr_t)d_outputs | (uintptr_t)d_status) & 3) return SH_ERR_INVALID;  // 32-bit reads
  VbPlan p;
  SH_TRY(vb_plan_stark_proof(&p, steps, ext, width, term_exps, term_counts, samples));
  SH_TRY(enter(c));
  SH_TRY(stark_terms(c, width, term_coefs, term_exps, term_counts));
  return vb_launch(c, p, d_proof, nullptr, d_inputs, d_outputs, io_stride, batch, d_status);
}

int sh_dev_fri_verify(sh_ctx* c, const void* d_proof, const void* d_merkle_roots, uint64_t n, const uint8_t root[32], uint64_t maxdeg_plus_1,
                      uint32_t exclude_multiples_of, uint32_t samples, uint32_t batch, int32_t* d_status) {
  if (!c || !d_proof || !d_merkle_roots || !d_status || batch == 0) return SH_ERR_INVALID;
  if (((uintptr_t)d_proof | (uintptr_t)d_merkle_roots | (uintptr_t)d_status) & 3) return SH_ERR_INVALID;  // read as 32-bit words
  VbPlan p;
  SH_TRY(vb_plan_fri_proof(&p, n, root, maxdeg_plus_1, exclude_multiples_of, samples));
  SH_TRY(enter(c));
  return vb_launch(c, p, d_proof, d_merkle_roots, nullptr, nullptr, 0, batch, d_status);
}

int sh_stark_verify_batch(sh_ctx* c, const uint8_t* proofs, uint64_t proof_len, const uint8_t* inputs, const uint8_t* outputs, uint64_t steps,
                          uint32_t ext, uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts,
                          uint32_t samples, uint32_t batch, int32_t* status) {
  if (!c || !proofs || !inputs || !outputs || !status || !term_coefs || batch == 0) return SH_ERR_INVALID;
  VbPlan p;
  SH_TRY(vb_plan_stark_proof(&p, steps, ext, width, term_exps, term_counts, samples));
  if (proof_len != p.plen) {  // the host verifier's decision on each mis-sized proof; nothing is launched
    for (uint32_t b = 0; b < batch; ++b)
      status[b] = sh_stark_verify(proofs + (size_t)b * proof_len, proof_len, inputs + 32ull * width * b, outputs + 32ull * width * b, steps,
                                  ext, width, term_coefs, term_exps, term_counts, samples);
    return SH_ERR_INVALID;
  }
  SH_TRY(enter(c));
  SH_TRY(stark_terms(c, width, term_coefs, term_exps, term_counts));
  const size_t pbytes = vb_round_up((size_t)batch * proof_len), io = vb_round_up((size_t)batch * width * sizeof(fp));
  void *ws = nullptr, *wire = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_VB_IO, pbytes + 2 * io + (size_t)batch * 4, &ws));
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, 2 * io, &wire));
  uint8_t* d = static_cast<uint8_t*>(ws);
  fp* d_in = reinterpret_cast<fp*>(d + pbytes);
  fp* d_out = reinterpret_cast<fp*>(d + pbytes + io);
  int32_t* d_status = reinterpret_cast<int32_t*>(d + pbytes + 2 * io);
  uint8_t* w = static_cast<uint8_t*>(wire);
  SH_TRY(h2d(c, d, proofs, (size_t)batch * proof_len));
  SH_TRY(h2d(c, w, inputs, (size_t)batch * width * 32));
  SH_TRY(h2d(c, w + io, outputs, (size_t)batch * width * 32));
  HIP_TRY(c, shk_wire_to_limb(w, d_in, (uint64_t)batch * width, c->stream));
  HIP_TRY(c, shk_wire_to_limb(w + io, d_out, (uint64_t)batch * width, c->stream));
  SH_TRY(vb_launch(c, p, d, nullptr, d_in, d_out, 1, batch, d_status));
  return d2h(c, status, d_status, (size_t)batch * 4);
}

int sh_fri_verify_batch(sh_ctx* c, const uint8_t* proofs, uint64_t proof_len, const uint8_t* merkle_roots, uint64_t n, const uint8_t root[32],
                        uint64_t maxdeg_plus_1, uint32_t exclude_multiples_of, uint32_t samples, uint32_t batch, int32_t* status) {
  if (!c || !proofs || !merkle_roots || !status || batch == 0) return SH_ERR_INVALID;
  VbPlan p;
  SH_TRY(vb_plan_fri_proof(&p, n, root, maxdeg_plus_1, exclude_multiples_of, samples));
  if (proof_len != p.plen) {
    for (uint32_t b = 0; b < batch; ++b)
      status[b] = sh_fri_verify(proofs + (size_t)b * proof_len, proof_len, merkle_roots + 32ull * b, n, root, maxdeg_plus_1,
                                exclude_multiples_of, samples);
    return SH_ERR_INVALID;
  }
  SH_TRY(enter(c));
  const size_t pbytes = vb_round_up((size_t)batch * proof_len), rbytes = vb_round_up((size_t)batch * 32);
  void* ws = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_VB_IO, pbytes + rbytes + (size_t)batch * 4, &ws));
  uint8_t* d = static_cast<uint8_t*>(ws);
  int32_t* d_status = reinterpret_cast<int32_t*>(d + pbytes + rbytes);
  SH_TRY(h2d(c, d, proofs, (size_t)batch * proof_len));
  SH_TRY(h2d(c, d + pbytes, merkle_roots, (size_t)batch * 32));
  SH_TRY(vb_launch(c, p, d, d + pbytes, nullptr, nullptr, 0, batch, d_status));
  return d2h(c, status, d_status, (size_t)batch * 4);
}
}  // extern "C"
