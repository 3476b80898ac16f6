"""The witness side of the prover: `get_computational_trace` and the parts of `AIR` that `STARK.mk_proof`'s callers
use (starks/air.py:32-52, 94-131): `generate_witness()` and `generate_boundary_constraints()`.

Host-side glue on Python ints.  One deliberate difference: the reference's constructor asserts `steps == 2**9 - 1`
(air.py:94), which contradicts every STARK call site in its own tests (steps 8 / 32 / 512, test_stark.py:215-350) and
the power-of-two domain `STARK` needs (stark.py:205-208); that assert and the monotone-circuit bookkeeping
(air.py:113-118, 133-160) are not mirrored.
"""


def get_computational_trace(inp, steps, width, step_polys):
    """air.py:32-52 -> (trace, output); trace[step][dim]."""
    trace = [list(inp)]
    for _ in range(steps - 1):
        trace.append([step_polys[i](trace[-1]) for i in range(width)])
    return trace, trace[-1]


def device_witness(field, inp, steps, step_polys):
    """AIR(...).generate_witness() on the GPU: witness[dim] as one WireList of `steps` elements of `field` per dimension.  The MiMC
    field goes through sh_stark_witness, any other odd modulus below 2^256 through sh_mod_stark_witness (stark.witness_flat /
    stark.mod_witness_flat); inputs may be ints or field elements.  `AIR` itself stays host-side Python."""
    from . import stark
    from ._lib import MIMC_P
    from .wireseq import WireList
    if isinstance(inp, int):  # air.py:89-90
        inp = [inp]
    p, width = int(field.p), len(step_polys)
    if len(inp) != width:
        raise ValueError("%d inputs for %d step polynomials" % (len(inp), width))
    raw = b"".join((int(v) % p).to_bytes(32, "big") for v in inp)
    if p == MIMC_P:
        flat = stark.witness_flat(raw, steps, width, step_polys)
    else:
        if p < 3 or p % 2 == 0 or p >> 256:
            raise NotImplementedError("device_witness takes odd moduli 3 <= p < 2^256 (got %d)" % p)
        flat = stark.mod_witness_flat(p, raw, steps, width, step_polys)
    return [WireList(flat[32 * steps * d:32 * steps * (d + 1)], field) for d in range(width)]


class AIR(object):
    def __init__(self, field, width, inp, steps, step_polys, extension_factor):
        self.field = field
        self.width = width
        if isinstance(inp, int):  # air.py:89-90
            inp = [inp]
        self.inp = [field(v) for v in inp]
        self.steps = steps
        self.step_polys = step_polys
        self.extension_factor = extension_factor
        self.computational_trace, self.output = get_computational_trace(self.inp, steps, width, step_polys)
        self.F, self.T, self.w = field, steps, width

    def generate_witness(self):
        """air.py:121-123: witness[dim][step]"""
        return [[self.computational_trace[i][j] for i in range(self.steps)] for j in range(self.w)]

    def generate_boundary_constraints(self):
        """air.py:125-131: (step 0, dim, input value)"""
        return [(0, ind, self.inp[ind]) for ind in range(self.w)]

    def get_degree(self):
        return max(poly.degree() for poly in self.step_polys)
