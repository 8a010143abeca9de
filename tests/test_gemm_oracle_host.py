"""CPU checks of oracle/gemm_ref.py, the float64 oracle tests/test_gpu_gemm_oracle.py holds cvar_gemm to:
  - the numpy float32 model of the kernels' arithmetic (chunked accumulation, the epilogue steps in order, bf16 roundings) stays at <= 0.5 of the
    bound on every element of every tensor a case writes - a correct kernel can pass.  A bf16 tensor's half-ulp store term IS the worst case of its
    rounding: the model before that rounding is held to 0.5 of the bound without the term, the rounded model to the whole bound;
  - arithmetic-only faults planted in the model land outside the bound, on at least one element, for every case that uses the affected flag -
    a condition on the operands chosen in the case table, not a tolerance.  The share of elements each fault moves outside is printed.
"""
import numpy as np
import pytest

from oracle import gemm_ref as G

NAMES = list(G.CASES)
_ACC = {}


def acc_of(c):
    """the fault-free accumulators of a case, shared by the model and by every fault that leaves the K loop alone"""
    if c.name not in _ACC:
        _ACC[c.name] = G._accumulate(c, G.operands(c), None)
    return _ACC[c.name]


def tensors(c, md, ev):
    """(tensor, model value, reference, bound) of everything the call writes; C as the memory image (remapped rows, NaN where nothing is owned)"""
    ref_img, _ = G.image(c, ev.C)
    bnd_img, _ = G.image(c, ev.C_bound)
    got_img, spare = G.image(c, md.C, md.rows)
    out = [('C', got_img, ref_img, bnd_img)]
    if not np.isnan(spare).all():            # something landed past the arena
        out.append(('C past the arena', np.where(np.isnan(spare), np.nan, np.inf), np.full(spare.shape, np.nan), np.zeros(spare.shape)))
    if c.split_n:
        out.append(('C_split', md.Cs, ev.Cs, ev.Cs_bound))
    if c.pre_act:
        out.append(('pre_act', md.pre, ev.pre, ev.pre_bound))
    return out


def test_case_table_is_consistent():
    assert len(NAMES) >= 100
    for c in G.CASES.values():
        assert c.K % (8 if c.dt == 'bf16' else 4) == 0, c.name
        if c.split_n:
            assert c.remap and c.batch == 1 and not c.res and not c.gate_rows and c.act == G.ACT_NONE, c.name      # what cvar_gemm accepts
            assert c.split_n % 8 == 0 and c.N % 8 == 0 and c.ld_split % 8 == 0 and c.ldc % 8 == 0, c.name
        if c.pre_act or c.act == G.ACT_GELU_GRAD:
            assert not c.remap and not c.small_m, c.name
        if c.ln:
            assert c.gate_rows and c.res == 'f32' and c.inplace and c.out == 'f32' and c.ldc == c.N and c.ldr == c.N, c.name
    for f in G.FAULTS:
        assert sum(G.uses(c, f) for c in G.CASES.values()) >= 4, f
    for impl in (G.SPEC, G.RPF, G.VEC, G.SCALAR, G.QUAD_SK, G.QUAD_ST, G.ROWFIN):
        assert any(c.impl == impl for c in G.CASES.values()), impl


def test_number_formats():
    x = np.array([1.0, 1.00390625, 1.005859375, 1.01171875, -3.0e-5, 257.0], dtype=np.float32)
    r = G.bf16_round(x)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == 1.0078125 and r[3] == 1.015625      # ties to even: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert np.all(np.abs(r.astype(np.float64) - x) <= G.bf16_half_ulp(np.abs(x)))
    assert abs(float(r[1]) - float(x[1])) > G.BF16_STORE * float(x[1])           # a correct rounding that 2^-9 |value| would refuse
    assert np.all(G.bf16_half_ulp(np.abs(x)) <= 2 * G.BF16_STORE * np.abs(x)) and G.bf16_half_ulp(1.9999) < 1.0001 * G.BF16_STORE * 2
    assert np.all(np.abs(G.bf16_trunc(x)) <= np.abs(x))
    t = np.linspace(-8, 8, 4001)
    y, _ = G._gelu64(t)
    gp, _ = G._gelu_grad64(t)
    assert np.max(np.abs(y - 0.5 * t * (1 + np.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3))))) < 1e-14
    assert np.max(np.abs(gp - np.gradient(y, t))[2:-2]) < 1e-4 and np.max(np.abs(gp)) <= G.GELU_LIP


@pytest.mark.parametrize('name', NAMES)
def test_model_within_half_the_bound(name):
    c = G.CASES[name]
    ev = G.evaluate(c)
    md = G.model(c, acc=acc_of(c))
    raws = [('C', md.C_raw, ev.C, ev.C_raw_bound)]
    if c.split_n:
        raws.append(('C_split', md.Cs_raw, ev.Cs, ev.Cs_raw_bound))
    if c.pre_act:
        raws.append(('pre_act', md.pre_raw, ev.pre, ev.pre_raw_bound))
    for tensor, got, ref, bnd in raws:
        assert got.shape == ref.shape == bnd.shape, (name, tensor)
        r = G.ratio_of(G.abs_err(got, ref), bnd)
        print(f'[gemm_host] {name:28s} {tensor:8s} model before the store / bound {r:6.3f}')
        assert r <= 0.5, (name, tensor, r)
    for tensor, got, ref, bnd in tensors(c, md, ev):
        r = G.ratio_of(G.abs_err(got, ref), bnd)
        print(f'[gemm_host] {name:28s} {tensor:8s} model as stored / whole bound  {r:6.3f}')
        stored_bf16 = (c.dt if tensor == 'pre_act' else c.out) == 'bf16'
        assert r <= (1.0 if stored_bf16 else 0.5), (name, tensor, r)


@pytest.mark.parametrize('fault', G.FAULTS)
def test_planted_fault_lands_outside_the_bound(fault):
    used = [c for c in G.CASES.values() if G.uses(c, fault)]
    assert used
    missed = []
    for c in used:
        ev = G.evaluate(c)
        md = G.model(c, fault, acc=None if fault.startswith('drop_') else acc_of(c))
        share = {t: G.outside_share(G.abs_err(got, ref), bnd) for t, got, ref, bnd in tensors(c, md, ev)}
        print(f'[gemm_host] {fault:18s} {c.name:28s} share of elements outside: ' + '  '.join(f'{t} {s:.3f}' for t, s in share.items()))
        if not max(share.values()) > 0:
            missed.append(c.name)
    assert not missed, (fault, missed)
