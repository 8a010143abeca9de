"""The hot-path kernels at the shapes of the headline run (d24 autoregressive_infer_cfg, bf16, B = 512 per GPU), where tensors cross 2^31 / 2^32
bytes and elements, and a whole depth-2 generation at B = 512 with 512 different rows.

At B = 512 the last scale of the pyramid runs R = 1024 sequences x l = 512 new tokens = M = 524 288 rows through every transformer kernel:

    tensor                               shape, dtype                    first row behind the boundary
    residual stream x                    (M, 1536) fp32                  2^31 bytes: row 349 525
    hbuf (fc1 out, fc2 in)               (M, 6144) bf16                  2^31 bytes: row 174 762;  2^31 elements = 2^32 bytes: row 349 525
    logits                               (M, 4096) fp32                  2^31 bytes: row 131 072;  2^32 bytes: row 262 144
    one layer of the K/V arena           (1024, 1360, 3072) bf16         2^31 bytes: sequence 257;  2^31 elements = 2^32 bytes: sequence 514
    arena layer i >= 1                   base + i * 4.28e9 elements      (the wrappers fold the layer offset into the pointer)
    CFG-combined logits                  (512 * 512, 4096) fp32          2^31 bytes: row 131 072
    decoder activations, 128 images      (128 * 65536, 160) bf16         2^31 bytes: image 102

(the rows are computed from the shapes by `boundary_rows`; the CPU test below pins them to this table).  Part 1 runs each call once at that shape, on
non-periodic device-generated data, into NaN-prefilled outputs with NaN fences on both sides, and checks it twice:

  windows   the first 512 rows, the last 512 rows and 512 rows centred on every boundary row of every tensor the op indexes are copied to the host
            and compared with a float64 computation on the stored operands, at the bound the small-shape test of the same op asserts;
  whole     the same op runs again as 8 row chunks (65 536 rows each: below every boundary, the regime the rest of the suite pins) and the big result is
            compared with them over ALL rows on the device.  Every comparison is torch.equal: none of these ops sums a row in an order that depends
            on M at M >= 65 536 (GEMMs: unsliced 256x256 tiles for both sizes, one K order per output; attention / cos-norm: one workgroup or
            wave per (sequence, head, block); LayerNorm, word_embed, cfg_sample: one row per wave / thread / workgroup).

Part 2 generates 512 different (label, condition type) samples with a depth-2 model of d24 width (the kernels and row counts of the headline, two arena
layers) and compares seven of them with the same seven generated alone.  What is still only exercised by bench.py: the full 24-layer arena (205 GB).

Peak device memory is derived from the shapes in a comment at each test; the largest are the arena tests (~32 GB) and Part 2 (~60 GB)."""
import math

import pytest
import torch
import torch.nn.functional as F

from controlvar_amd import ops
from controlvar_amd._lib import ACT_GELU_TANH, ACT_NONE
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, Pyramid, VarConfig

F32, BF16 = torch.float32, torch.bfloat16
TWO31, TWO32 = 1 << 31, 1 << 32

# ---- the headline shapes: d24 at B = 512, last scale
B_HEAD = 512
CFG24 = VarConfig(depth=24)
PY = Pyramid()
C, H, V = CFG24.C, CFG24.H, CFG24.vocab                     # 1536, 24, 4096
HID = 4 * C                                                 # 6144
R = 2 * B_HEAD                                              # CFG: [cond ; uncond] sequences
L_LAST, Q_OFF, LMAX = PY.l[-1], PY.begin[-1], PY.L          # 512 new tokens at offset 848 of 1360
M = R * L_LAST                                              # 524 288 rows
N_ADA = CFG24.depth * 6 * C + 2 * C                         # width of the adaLN table (models.ControlVAR._build_pack)
LATE_BLOCK = CFG24.depth - 1                                # gates / modulations of the last block: read far from the start of the table
ARENA_STRIDE = R * LMAX * 2 * C                             # elements of one layer of the K/V arena
NCHUNK = 8
WINDOW = 512
DECODE_CHUNK, DEC_HW, DEC_CH = 128, 256 * 256, 160          # models.VQVAE.decode_chunk images of 256 x 256 pixels x ch 160 in front of conv_out
VAE_PICKS = (0, 101, 102, 103, 127)
ARENA_SEQS_REQUIRED = (0, 513, 514, 515, 1023)
GEN_PICKS = (0, 1, 2, 3, 255, 256, 511)                     # sample 2's unconditional partner is sequence 514


# ------------------------------------------------------------------------------------------------ plain helpers (run on the CPU as well)
def boundary_rows(rows: int, width: int, esize: int) -> dict:
    """{boundary name: row that holds the first element behind it} for a dense (rows, width) tensor of esize-byte elements; boundaries the tensor
    does not reach are left out"""
    out = {}
    for name, elems in (('2^31 bytes', TWO31 // esize), ('2^32 bytes', TWO32 // esize), ('2^31 elements', TWO31), ('2^32 elements', TWO32)):
        if elems < rows * width:
            out[name] = elems // width
    return out


def row_windows(rows: int, brows, size: int = WINDOW):
    """merged [lo, hi) row ranges: the first `size` rows, the last `size` rows and `size` rows centred on every boundary row"""
    spans = [(0, min(size, rows)), (max(rows - size, 0), rows)]
    spans += [(max(r - size // 2, 0), min(r + size // 2, rows)) for r in brows]
    spans.sort()
    merged = [list(spans[0])]
    for lo, hi in spans[1:]:
        if lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    return [tuple(s) for s in merged]


def in_windows(windows, row: int) -> bool:
    return any(lo <= row < hi for lo, hi in windows)


def chunk_bounds(rows: int, n: int = NCHUNK, unit: int = 1):
    """n consecutive [lo, hi) chunks of rows // n rows (a multiple of `unit`); the last one takes the remainder"""
    step = rows // n // unit * unit
    return [(i * step, (i + 1) * step if i + 1 < n else rows) for i in range(n)]


def failing_windows(fetch, reference, windows, accept):
    """fetch(lo, hi) -> host copy of result rows [lo, hi); reference(lo, hi) -> the float64 reference of those rows; accept(got, ref) -> bool.
    Returns the windows that are not finite or not accepted."""
    bad = []
    for lo, hi in windows:
        got, ref = fetch(lo, hi), reference(lo, hi)
        if not (bool(torch.isfinite(got.double()).all()) and bool(accept(got, ref))):
            bad.append((lo, hi))
    return bad


def failing_chunks(big, parts, rows: int, same=torch.equal):
    """parts: [(lo, hi, result of rows [lo, hi) computed on their own)], which must tile [0, rows) without a gap.  Returns the chunks of `big`
    that differ from their part or hold a non-finite value."""
    bad, at = [], 0
    for lo, hi, small in parts:
        assert lo == at and hi > lo, 'the chunks must cover every row once'
        at = hi
        sl = big[lo:hi]
        if not (bool(torch.isfinite(sl).all()) and same(sl, small)):
            bad.append((lo, hi))
    assert at == rows, 'the chunks must cover every row once'
    return bad


def gate_off_of(block: int, which: int) -> int:
    """element offset of adaLN vector `which` (0 gamma1, 1 gamma2, 2 scale1, 3 scale2, 4 shift1, 5 shift2) of a block inside a row of the table"""
    return block * 6 * C + which * C


# ------------------------------------------------------------------------------------------------ CPU: the windows cover the table, the helpers can fail
def test_every_boundary_row_lies_inside_a_window_and_the_checks_go_red():
    """From the shapes alone: the boundary rows are the ones in the module docstring, each lies inside a window of its op, the arena / decoder
    boundaries fall inside the sequences / images the tests take, and the chunks of the whole-tensor comparison stay below every boundary.
    Then the two helpers on a small synthetic result: a row copied over the row a fixed distance later (an aliased write) and a zeroed row (a
    clamped buffer range) turn both checks red."""
    assert (C, H, V, HID, R, L_LAST, Q_OFF, LMAX, M) == (1536, 24, 4096, 6144, 1024, 512, 848, 1360, 524288)
    x_b, h_b, lg_b = boundary_rows(M, C, 4), boundary_rows(M, HID, 2), boundary_rows(M, V, 4)
    assert x_b == {'2^31 bytes': 349525}
    assert h_b == {'2^31 bytes': 174762, '2^32 bytes': 349525, '2^31 elements': 349525}
    assert lg_b == {'2^31 bytes': 131072, '2^32 bytes': 262144}              # exactly 2^31 elements: the count itself no longer fits an int
    assert M * V == TWO31
    assert boundary_rows(M, C, 2) == {}                                       # u, o, qs: 1.6e9 bytes
    comb_b = boundary_rows(B_HEAD * L_LAST, V, 4)
    assert comb_b == {'2^31 bytes': 131072} and B_HEAD * L_LAST * V * 4 == TWO32
    arena_b = boundary_rows(R, LMAX * 2 * C, 2)
    assert arena_b == {'2^31 bytes': 257, '2^32 bytes': 514, '2^31 elements': 514}
    assert TWO31 < ARENA_STRIDE < TWO32 < 2 * ARENA_STRIDE             # layer 1 begins 4.28e9 elements = 8.6e9 bytes behind the arena's base and crosses 2^32 elements
    dec_b = boundary_rows(DECODE_CHUNK, DEC_HW * DEC_CH, 2)
    assert dec_b == {'2^31 bytes': 102}
    for op, tensors in _OP_TENSORS.items():
        win = row_windows(_OP_ROWS[op], _op_boundary_rows(op))
        assert in_windows(win, 0) and in_windows(win, _OP_ROWS[op] - 1), op
        for rows, width, esize in tensors:
            for name, r in boundary_rows(rows, width, esize).items():
                r = r % _OP_ROWS[op]                                          # cfg_sample: logits rows of the unconditional half fold onto the combined rows
                assert all(in_windows(win, rr) for rr in (max(r - 1, 0), r, min(r + 1, _OP_ROWS[op] - 1))), (op, name, r)
                if r not in (0, _OP_ROWS[op] - 1):
                    assert any(lo <= r - 128 and r + 128 <= hi for lo, hi in win), (op, name, r)      # a full 256-row tile on either side
    seqs = arena_sequences()
    assert set(ARENA_SEQS_REQUIRED) <= set(seqs)
    for s in arena_b.values():
        assert {s - 1, s, s + 1} <= set(seqs)
    for b in dec_b.values():
        assert {b - 1, b, b + 1} <= set(VAE_PICKS)
    assert {0, DECODE_CHUNK - 1} <= set(VAE_PICKS)
    assert (2 + B_HEAD) in arena_b.values() and 2 in GEN_PICKS              # generation: sample 2's unconditional sequence straddles 2^31 elements
    # every chunk of the whole-tensor comparison lies below all boundaries
    for rows, width, esize in [(M + 37, HID, 2), (M, V, 4), (M, C, 4)]:
        for lo, hi in chunk_bounds(rows, unit=L_LAST):
            assert (hi - lo) * width * esize < TWO31 and (hi - lo) * width < TWO31
    assert chunk_bounds(M + 37, unit=L_LAST)[-1] == (7 * 65536, M + 37) and chunk_bounds(M) == [(i * 65536, (i + 1) * 65536) for i in range(8)]
    assert (R // NCHUNK) * LMAX * 2 * C * 2 < TWO31

    # ---- the helpers on a synthetic result
    g = torch.Generator().manual_seed(3)
    rows, width, brow, dist = 4096, 64, 2731, 1024
    a, w = torch.randn(rows, 16, generator=g), torch.randn(width, 16, generator=g)
    good = (a @ w.t()).contiguous()
    win = row_windows(rows, [brow], size=64)
    assert win == [(0, 64), (brow - 32, brow + 32), (rows - 64, rows)]
    parts = [(lo, hi, (a[lo:hi] @ w.t()).contiguous()) for lo, hi in chunk_bounds(rows)]

    def checks(res):
        acc = lambda got, ref: bool(((got.double() - ref).abs() <= 1e-4 * (ref.abs() + 1)).all())
        fw = failing_windows(lambda lo, hi: res[lo:hi].clone(), lambda lo, hi: a[lo:hi].double() @ w.double().t(), win, acc)
        return fw, failing_chunks(res, parts, rows, same=lambda p, q: bool(((p - q).abs() <= 1e-5).all()))

    assert checks(good) == ([], [])
    aliased = good.clone()
    aliased[brow] = good[brow - dist]                       # the write of row brow - dist landed on row brow as well
    assert checks(aliased) == ([(brow - 32, brow + 32)], [(2560, 3072)])
    zeroed = good.clone()
    zeroed[brow + 1] = 0.0                                  # a store / load beyond a clamped buffer range: dropped / zeros
    assert checks(zeroed) == ([(brow - 32, brow + 32)], [(2560, 3072)])
    nan = good.clone()
    nan[5, 7] = float('nan')                                # a row the kernel never wrote
    assert checks(nan) == ([(0, 64)], [(0, 512)])
    outside = good.clone()
    outside[1500] = good[1500 - dist]                       # outside every window: only the whole-tensor comparison can see it
    assert checks(outside) == ([], [(1024, 1536)])
    with pytest.raises(AssertionError):
        failing_chunks(good, parts[:-1], rows)              # a comparison that leaves rows out is itself an error


# tensors each op indexes by row at the headline shape: (rows, width, element size)
_OP_ROWS = {'ln_modulate': M, 'proj': M, 'fc1': M, 'fc1_ragged': M + 37, 'fc2': M, 'head': M, 'cfg_sample': B_HEAD * L_LAST, 'word_embed': M}
_OP_TENSORS = {
    'ln_modulate': [(M, C, 4), (M, C, 2)],
    'proj': [(M, C, 2), (M, C, 4)],
    'fc1': [(M, C, 2), (M, HID, 2)],
    'fc1_ragged': [(M + 37, C, 2), (M + 37, HID, 2)],
    'fc2': [(M, HID, 2), (M, C, 4)],
    'head': [(M, C, 2), (M, V, 4)],
    'cfg_sample': [(M, V, 4), (B_HEAD * L_LAST, V, 4)],
    'word_embed': [(M, C, 4)],
}


def _op_boundary_rows(op):
    rows = set()
    for r, w, e in _OP_TENSORS[op]:
        rows |= {b % _OP_ROWS[op] for b in boundary_rows(r, w, e).values()}
    return sorted(rows)


def op_windows(op):
    return row_windows(_OP_ROWS[op], _op_boundary_rows(op))


def arena_sequences():
    """sequences whose rows get a float64 reference: the first, the last, and every sequence a boundary of one arena layer falls into, with its neighbours"""
    seqs = {0, R - 1}
    for s in boundary_rows(R, LMAX * 2 * C, 2).values():
        seqs |= {s - 1, s, s + 1}
    return sorted(seqs)


# ------------------------------------------------------------------------------------------------ device helpers
def need(dev, nbytes: int):
    """the one skip of a test: not enough free device memory for its derived peak (never on an MI355X, 288 GB)"""
    free, _ = torch.cuda.mem_get_info(dev)
    if free < nbytes:
        pytest.skip(f'needs {nbytes} bytes of free device memory, {free} available')


def release():
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def dev_randn(shape, dtype, dev, gen, std=1.0, mean=0.0, out=None):
    """seeded normal data generated on the device in pieces of at most 2^28 elements (nothing periodic: the generator runs on)"""
    t = torch.empty(shape, dtype=dtype, device=dev) if out is None else out
    flat = t.view(-1)
    step = 1 << 28
    for lo in range(0, flat.numel(), step):
        piece = flat[lo:lo + step]
        piece.normal_(mean, std, generator=gen)
    return t


FENCE = 4096        # elements: keeps the tensor 16-byte aligned


def fenced(shape, dtype, dev):
    """a NaN-filled tensor of `shape` with a NaN fence in front of and behind it; returns (buffer, view)"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * FENCE,), float('nan'), dtype=dtype, device=dev)
    return buf, buf[FENCE:FENCE + n].view(shape)


def fence_intact(buf) -> bool:
    return bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[-FENCE:]).all())


def all_finite(t) -> bool:
    flat = t.reshape(-1)
    return all(bool(torch.isfinite(flat[lo:lo + (1 << 29)]).all()) for lo in range(0, flat.numel(), 1 << 29))


def all_nan(t) -> bool:
    flat = t.reshape(-1)                  # callers pass contiguous views: no copy
    return all(bool(torch.isnan(flat[lo:lo + (1 << 29)]).all()) for lo in range(0, flat.numel(), 1 << 29))


def host64(t):
    return t.double().cpu()


# ------------------------------------------------------------------------------------------------ Part 1: one op at a time
@pytest.mark.gpu
def test_ln_modulate_at_the_headline_rows(gpu_device):
    """cvar_ln_modulate: x (M, 1536) fp32 -> bf16 with the last block's scale / shift out of the (1024, n_ada) table, 512 rows per table row.
    Peak: x 3.2 GB + ada 0.9 GB + out 1.6 GB + one chunk 0.2 GB = 6 GB."""
    from test_gpu_kernels import close
    dev = gpu_device
    need(dev, 8 << 30)
    g = torch.Generator(device=dev).manual_seed(101)
    x = dev_randn((M, C), F32, dev, g, std=2.0, mean=0.5)
    ada = dev_randn((R, N_ADA), F32, dev, g, std=0.3)
    sc_off, sh_off = gate_off_of(LATE_BLOCK, 3), gate_off_of(LATE_BLOCK, 5)
    buf, out = fenced((M, C), BF16, dev)
    ops.ln_modulate(x, ada, sc_off, sh_off, N_ADA, L_LAST, out, M, C, 1e-6)

    def reference(lo, hi):
        rows = torch.arange(lo, hi) // L_LAST
        a = host64(ada[lo // L_LAST:(hi - 1) // L_LAST + 1])[rows - lo // L_LAST]
        return F.layer_norm(host64(x[lo:hi]), (C,), eps=1e-6) * (1 + a[:, sc_off:sc_off + C]) + a[:, sh_off:sh_off + C]

    bad = failing_windows(lambda lo, hi: out[lo:hi].cpu(), reference, op_windows('ln_modulate'), lambda got, ref: close(got, ref, BF16, 2e-5))
    assert bad == [], bad
    for lo, hi in chunk_bounds(M, unit=L_LAST):
        small = torch.full((hi - lo, C), float('nan'), dtype=BF16, device=dev)
        ops.ln_modulate(x[lo:hi], ada[lo // L_LAST:hi // L_LAST], sc_off, sh_off, N_ADA, L_LAST, small, hi - lo, C, 1e-6)
        assert failing_chunks(out[lo:hi], [(0, hi - lo, small)], hi - lo) == [], (lo, hi)        # the chunks tile [0, M): chunk_bounds
        del small
    assert fence_intact(buf)
    del x, ada, buf, out
    release()


def _gemm_case(dev, op, *, N, K, act=ACT_NONE, out_dtype, gated_block=None, w_std, accept, seed):
    """one transformer GEMM at _OP_ROWS[op] rows: A (rows, K) bf16, W (N, K) bf16, fp32 bias; gated_block = (block, which): out is the fp32 residual
    stream, updated in place with that block's gate out of the (1024, n_ada) table.  Window check against float64, all rows against 8 chunked calls."""
    rows = _OP_ROWS[op]
    g = torch.Generator(device=dev).manual_seed(seed)
    A = dev_randn((rows, K), BF16, dev, g)
    W = dev_randn((N, K), BF16, dev, g, std=w_std)
    bias = dev_randn((N,), F32, dev, g)
    buf, out = fenced((rows, N), out_dtype, dev)
    kw = dict(N=N, K=K, bias=bias, act=act, small_m=True, split_k=True)        # as models.ControlVAR._blocks_and_head issues them (default plan)
    x0 = ada = None
    if gated_block is not None:
        ada = dev_randn(((rows + L_LAST - 1) // L_LAST, N_ADA), F32, dev, g, std=0.3)
        x0 = dev_randn((rows, N), F32, dev, g)
        out.copy_(x0)
        kw.update(gate=ada, gate_off=gate_off_of(*gated_block), ldg=N_ADA, gate_rows=L_LAST)
        ops.gemm(A, W, out, M=rows, residual=out, **kw)
    else:
        ops.gemm(A, W, out, M=rows, **kw)
    Wd, bd = host64(W), host64(bias)

    def reference(lo, hi):
        acc = host64(A[lo:hi]) @ Wd.t() + bd
        if act == ACT_GELU_TANH:
            acc = F.gelu(acc, approximate='tanh')
        if gated_block is not None:
            go = gate_off_of(*gated_block)
            r0 = lo // L_LAST
            gt = host64(ada[r0:(hi - 1) // L_LAST + 1, go:go + N])[torch.arange(lo, hi) // L_LAST - r0]
            acc = host64(x0[lo:hi]) + acc * gt
        return acc

    bad = failing_windows(lambda lo, hi: out[lo:hi].cpu(), reference, op_windows(op), accept)
    assert bad == [], (op, bad)
    for lo, hi in chunk_bounds(rows, unit=L_LAST):
        if gated_block is not None:
            small = x0[lo:hi].clone()
            ops.gemm(A[lo:hi], W, small, M=hi - lo, residual=small, **dict(kw, gate=ada[lo // L_LAST:(hi + L_LAST - 1) // L_LAST]))
        else:
            small = torch.full((hi - lo, N), float('nan'), dtype=out_dtype, device=dev)
            ops.gemm(A[lo:hi], W, small, M=hi - lo, **kw)
        assert failing_chunks(out[lo:hi], [(0, hi - lo, small)], hi - lo) == [], (op, lo, hi)      # the chunks tile [0, rows): chunk_bounds
        del small
    assert fence_intact(buf), op
    return out, buf


@pytest.mark.gpu
@pytest.mark.parametrize('op,K', [('proj', C), ('fc2', HID)])
def test_gated_residual_gemm_in_place_at_the_headline_rows(gpu_device, op, K):
    """proj (K = 1536) and fc2 (K = 6144, A = hbuf: 2^31 elements at row 349 525): x += gate * (A W^T + b) in place on the fp32 stream (M, 1536), gate_rows = 512,
    ldg = n_ada, gate_off of the last block.  Bound: test_gemm_epilogues / test_gemm_split_k (bf16 operands: 1e-2 (|ref| + 1)).
    Peak (fc2): hbuf 6.4 GB + x 3.2 GB + copy of x 3.2 GB + ada 0.9 GB + one chunk 0.4 GB = 14 GB."""
    from test_gpu_kernels import close
    need(gpu_device, 18 << 30)
    out, buf = _gemm_case(gpu_device, op, N=C, K=K, out_dtype=F32, gated_block=(LATE_BLOCK, 0 if op == 'proj' else 1), w_std=1.0 / math.sqrt(K),
                          accept=lambda got, ref: close(got, ref, BF16, 3e-4), seed=103 if op == 'proj' else 105)
    del out, buf
    release()


@pytest.mark.gpu
@pytest.mark.parametrize('op', ['fc1', 'fc1_ragged'])
def test_fc1_gelu_gemm_at_the_headline_rows(gpu_device, op):
    """fc1: gelu_tanh(u W^T + b) -> hbuf (M, 6144) bf16, which crosses 2^31 bytes, 2^31 elements and 2^32 bytes; the ragged case has 37 more rows, so the
    last tile is partial at an offset beyond 2^32 bytes.  Bound: close() of test_gemm_epilogues.  Peak: hbuf 6.4 GB + u 1.6 GB + one chunk 0.8 GB = 9 GB."""
    from test_gpu_kernels import close
    need(gpu_device, 12 << 30)
    out, buf = _gemm_case(gpu_device, op, N=HID, K=C, act=ACT_GELU_TANH, out_dtype=BF16, w_std=1.0 / math.sqrt(C),
                          accept=lambda got, ref: close(got, ref, BF16), seed=104)
    del out, buf
    release()


@pytest.mark.gpu
def test_head_gemm_at_the_headline_rows(gpu_device):
    """head: u W^T + b -> logits (M, 4096) fp32: 2^31 elements, 2^33 bytes.  Bound: the sqrt(K) rule of test_gemm_plain.
    Peak: logits 8.6 GB + u 1.6 GB + one chunk 1.1 GB = 11.5 GB."""
    need(gpu_device, 14 << 30)
    out, buf = _gemm_case(gpu_device, 'head', N=V, K=C, out_dtype=F32, w_std=1.0,
                          accept=lambda got, ref: float((got.double() - ref).abs().max()) < 2e-3 * math.sqrt(C), seed=106)
    del out, buf
    release()


@pytest.mark.gpu
def test_ada_gemm_at_1024_sequences(gpu_device):
    """The adaLN table GEMM (models.ControlVAR._ada) at R = 1024: silu(cond) (1024, 1536) bf16 x w_ada (n_ada = 224 256, 1536) bf16 -> fp32, against float64 on
    sampled columns blocks (first, last, and the block around every 16 384th column).
    The narrowings to int of the small-M kernels, and the shape of this model that comes closest to 2 GiB for each (none reaches it, so none gets a large-side
    case here; cvar_gemm_skinny_plan refuses such a shape and the call stays on the tile kernels):
      gemm_skinny.hip  (int)(M * lda * 2), M <= 256: A = hbuf at fc2, 256 x 6144 x 2 = 3.1 MB;  (int)(N * ldw * 2): W = w_ada, 224 256 x 1536 x 2 = 0.69 GB (d30: 0.89 GB x 1.25 = 1.3 GB);
      gemm.hip         W's buffer range min(w_bytes, 0x7fffffff): the same w_ada, 0.69 GB; the split-K workspace is 256 MB by construction.
    Peak: w_ada 0.7 GB + ada 0.9 GB."""
    dev = gpu_device
    need(dev, 3 << 30)
    assert N_ADA * C * 2 < TWO31 and 256 * HID * 2 < TWO31
    g = torch.Generator(device=dev).manual_seed(107)
    cs = dev_randn((R, C), BF16, dev, g)
    W = dev_randn((N_ADA, C), BF16, dev, g, std=1.0)
    bias = dev_randn((N_ADA,), F32, dev, g)
    buf, ada = fenced((R, N_ADA), F32, dev)
    ops.gemm(cs, W, ada, M=R, N=N_ADA, K=C, bias=bias, small_m=True, split_k=True)
    assert all_finite(ada) and fence_intact(buf)
    csd = host64(cs)
    for n0 in sorted({0, N_ADA - 256} | set(range(16384 - 128, N_ADA - 256, 16384))):
        ref = csd @ host64(W[n0:n0 + 256]).t() + host64(bias[n0:n0 + 256])
        err = float((host64(ada[:, n0:n0 + 256]) - ref).abs().max())
        assert err < 2e-3 * math.sqrt(C), (n0, err)                            # test_gemm_plain
    del cs, W, bias, buf, ada
    release()


@pytest.mark.gpu
def test_qkv_gemm_writes_layer_1_of_a_two_layer_arena(gpu_device):
    """The qkv GEMM of inference: u (M, 1536) x w_qkv (4608, 1536) with remap = (512, 1360, 848), the q columns (x scale * log2 e) to their own (M, 1536)
    buffer, k | v into layer 1 of a [2][1024][1360][3072] bf16 arena (c_off = one layer = 4.28e9 elements; inside the layer 2^31 bytes falls into
    sequence 257, 2^31 elements into sequence 514).  Layer 0 and every arena row outside [848, 1360) must stay NaN.
    Bound: close() as in test_gemm_column_split_equals_the_unsplit_remap.  Peak: arena 17.1 GB + u 1.6 GB + q 1.6 GB + one chunk 1.3 GB = 22 GB."""
    from test_gpu_kernels import close
    dev = gpu_device
    need(dev, 26 << 30)
    g = torch.Generator(device=dev).manual_seed(108)
    u = dev_randn((M, C), BF16, dev, g)
    W = dev_randn((3 * C, C), BF16, dev, g, std=1.0 / math.sqrt(C))
    bias = dev_randn((3 * C,), F32, dev, g)
    abuf, arena = fenced((2, R, LMAX, 2 * C), BF16, dev)
    qbuf, qs = fenced((M, C), BF16, dev)
    alpha = float(CFG24.attn_scale) * 1.4426950408889634
    kw = dict(N=3 * C, K=C, bias=bias, ldc=2 * C, remap=(L_LAST, LMAX, Q_OFF), split_alpha=alpha, small_m=True, split_k=True)
    ops.gemm(u, W, arena, M=M, c_off=ARENA_STRIDE, split=(qs, C, C), **kw)
    assert all_nan(arena[0]), 'layer 0 was written'
    nseq = R // NCHUNK
    for s0 in range(0, R, nseq):
        lay = arena[1, s0:s0 + nseq]
        assert bool(torch.isnan(lay[:, :Q_OFF]).all()) and bool(torch.isnan(lay[:, Q_OFF + L_LAST:]).all()), f'rows of other scales written, sequences {s0}..'
    assert fence_intact(abuf) and fence_intact(qbuf)
    Wd, bd = host64(W), host64(bias)
    for s in arena_sequences():
        ref = host64(u[s * L_LAST:(s + 1) * L_LAST]) @ Wd.t() + bd
        got_q, got_kv = qs[s * L_LAST:(s + 1) * L_LAST].cpu(), arena[1, s, Q_OFF:Q_OFF + L_LAST].cpu()
        assert bool(torch.isfinite(got_q.float()).all()) and bool(torch.isfinite(got_kv.float()).all()), s
        assert close(got_q, ref[:, :C] * alpha, BF16, 2e-4), s
        assert close(got_kv, ref[:, C:], BF16, 2e-4), s
    for s0 in range(0, R, nseq):
        small = torch.full((nseq, LMAX, 2 * C), float('nan'), dtype=BF16, device=dev)
        sq = torch.full((nseq * L_LAST, C), float('nan'), dtype=BF16, device=dev)
        ops.gemm(u[s0 * L_LAST:(s0 + nseq) * L_LAST], W, small, M=nseq * L_LAST, split=(sq, C, C), **kw)
        assert failing_chunks(qs[s0 * L_LAST:(s0 + nseq) * L_LAST], [(0, nseq * L_LAST, sq)], nseq * L_LAST) == [], s0
        assert failing_chunks(arena[1, s0:s0 + nseq, Q_OFF:Q_OFF + L_LAST], [(0, nseq, small[:, Q_OFF:Q_OFF + L_LAST])], nseq) == [], s0
        del small, sq
    del u, W, abuf, arena, qbuf, qs
    release()


def _attention_reference(q, kv, log2_domain, scale):
    """float64 softmax attention of one sequence: q (l, C), kv (kvlen, 2C) as stored; no mask (inference: every cached key is visible)"""
    l, kvlen = q.shape[0], kv.shape[0]
    qh = q.double().view(l, H, 64).permute(1, 0, 2)
    kh = kv[:, :C].double().reshape(kvlen, H, 64).permute(1, 0, 2)
    vh = kv[:, C:].double().reshape(kvlen, H, 64).permute(1, 0, 2)
    s = qh @ kh.transpose(-1, -2) * (math.log(2.0) if log2_domain else scale)
    return (s.softmax(-1) @ vh).permute(1, 0, 2).reshape(l, C)


@pytest.mark.gpu
def test_attention_and_cos_qk_norm_on_layer_1_of_the_arena(gpu_device):
    """cvar_attention / cvar_attention_prescaled / cvar_cos_qk_norm in the K/V-arena form at qkv_off = one layer (4.28e9 elements), R = 1024, H = 24,
    q_off = 848, l = 512, Lmax = 1360: the prescaled bf16 form generation uses and the plain form against the float64 softmax of
    test_attention_mfma_flash_bf16 on the boundary sequences, all sequences against 8 chunked calls; then the cos-attention pre-pass (d30) in place.
    Layer 0 is NaN throughout: a read or a write that loses the layer offset shows.
    Peak: arena 17.1 GB + copy of layer 1 for the cos-norm 8.6 GB + q, q_pre, 2 outputs 6.4 GB + one chunk 1.3 GB = 33.5 GB."""
    from test_gpu_kernels import close
    dev = gpu_device
    need(dev, 38 << 30)
    g = torch.Generator(device=dev).manual_seed(109)
    abuf, arena = fenced((2, R, LMAX, 2 * C), BF16, dev)
    dev_randn(None, BF16, dev, g, out=arena[1])
    q = dev_randn((M, C), BF16, dev, g)
    scale = float(CFG24.attn_scale) * 4                       # the scores of unit-variance q, k then spread as the trained model's do (test_attention_mfma_flash_bf16)
    q_pre = (q.float() * (scale * 1.4426950408889634)).to(BF16)
    obuf, o_pre = fenced((M, C), BF16, dev)
    pbuf, o_plain = fenced((M, C), BF16, dev)
    ops.attention(arena, o_pre, R, H, LMAX, Q_OFF, L_LAST, scale, None, qkv_off=ARENA_STRIDE, q=q_pre, prescaled=True)
    ops.attention(arena, o_plain, R, H, LMAX, Q_OFF, L_LAST, scale, None, qkv_off=ARENA_STRIDE, q=q)
    assert all_finite(o_pre) and all_finite(o_plain) and fence_intact(obuf) and fence_intact(pbuf) and all_nan(arena[0])
    for s in arena_sequences():
        rows = slice(s * L_LAST, (s + 1) * L_LAST)
        kv = arena[1, s].cpu()
        ref_pre = _attention_reference(q_pre[rows].cpu(), kv, True, scale)
        ref_plain = _attention_reference(q[rows].cpu(), kv, False, scale)
        assert close(o_pre[rows], ref_pre, BF16, bf16_rel=2e-2), s
        assert close(o_plain[rows], ref_plain, BF16, bf16_rel=2e-2), s
    nseq = R // NCHUNK
    for s0 in range(0, R, nseq):
        rows = slice(s0 * L_LAST, (s0 + nseq) * L_LAST)
        for pre, big, qq in ((True, o_pre, q_pre), (False, o_plain, q)):
            small = torch.full((nseq * L_LAST, C), float('nan'), dtype=BF16, device=dev)
            ops.attention(arena[1, s0:s0 + nseq], small, nseq, H, LMAX, Q_OFF, L_LAST, scale, None, q=qq[rows], prescaled=pre)
            assert failing_chunks(big[rows], [(0, nseq * L_LAST, small)], nseq * L_LAST) == [], (s0, pre)
            del small
    del obuf, o_pre, pbuf, o_plain, q_pre, big, qq, kv
    release()
    # ---- cos-attention pre-pass in place: q <- normalize(q) e^sm q_mul, k rows [848, 1360) <- normalize(k); v and the other rows untouched
    before = arena[1].clone()
    q0 = q.clone()
    sm = torch.tensor([0.2 + 0.1 * i for i in range(2 * H)], device=dev)      # [depth][H] table: layer 1 reads the second row; the last heads hit the ln(100) clamp
    assert float(sm[-1]) > math.log(100) > float(sm[H])
    ops.cos_qk_norm(arena, R, H, LMAX, Q_OFF, L_LAST, sm, qkv_off=ARENA_STRIDE, sm_off=H, q=q, q_mul=1.4426950408889634)
    assert all_nan(arena[0]) and fence_intact(abuf)
    mul = host64(sm[H:]).clamp_max(math.log(100)).exp().view(1, H, 1) * 1.4426950408889634
    for s in arena_sequences():
        rows = slice(s * L_LAST, (s + 1) * L_LAST)
        ref_q = F.normalize(host64(q0[rows]).view(L_LAST, H, 64), dim=-1) * mul
        ref_k = F.normalize(host64(before[s, Q_OFF:, :C]).reshape(L_LAST, H, 64), dim=-1)
        assert close(q[rows].view(L_LAST, H, 64), ref_q, BF16, 1e-5, 1e-2), s
        assert close(arena[1, s, Q_OFF:, :C].reshape(L_LAST, H, 64), ref_k, BF16, 1e-5, 1e-2), s
    for s0 in range(0, R, nseq):
        rows = slice(s0 * L_LAST, (s0 + nseq) * L_LAST)
        small, sq = before[s0:s0 + nseq].clone(), q0[rows].clone()
        ops.cos_qk_norm(small, nseq, H, LMAX, Q_OFF, L_LAST, sm, sm_off=H, q=sq, q_mul=1.4426950408889634)
        assert failing_chunks(q[rows], [(0, nseq * L_LAST, sq)], nseq * L_LAST) == [], s0
        assert failing_chunks(arena[1, s0:s0 + nseq], [(0, nseq, small)], nseq) == [], s0          # v and the rows of other scales ride along: same bits as before
        assert torch.equal(small[:, :Q_OFF], before[s0:s0 + nseq, :Q_OFF]) and torch.equal(small[:, :, C:], before[s0:s0 + nseq, :, C:])
        del small, sq
    del abuf, arena, before, q, q0
    release()


@pytest.mark.gpu
def test_cfg_sample_at_the_headline_logits(gpu_device):
    """cvar_cfg_sample on logits [2 x 512][512][4096] fp32 (2^31 elements).  Greedy with the combined logits (2^32 bytes) and the margin: bit-exact on the
    windows against the CPU expression of test_cfg_greedy_and_combine, all 512 samples against 8 chunked calls over b.  One top-k 900 / top-p 0.96 call:
    on the window rows every draw lies inside the reference kept set and `kept` follows oracle.var_ref.topk_topp_mask_ within the +-1 rule of
    test_cfg_sample_topk_topp.  Peak: logits 8.6 GB + combined 4.3 GB + one chunk 1.1 + 0.5 GB = 14.5 GB."""
    from oracle.var_ref import topk_topp_mask_
    dev = gpu_device
    need(dev, 18 << 30)
    B, l = B_HEAD, L_LAST
    g = torch.Generator(device=dev).manual_seed(110)
    logits = dev_randn((2 * B, l, V), F32, dev, g, std=3.0)
    t = 4.0 * 3 / 9
    coef = [1 + t, -t]
    cbuf, comb = fenced((B, l, V), F32, dev)
    ibuf = torch.full((B * l + 2 * FENCE,), -1, dtype=torch.int32, device=dev)
    idx = ibuf[FENCE:FENCE + B * l].view(B, l)
    mbuf, mg = fenced((B, l), F32, dev)
    ops.cfg_sample(logits, B, 2, l, V, coef, 1, 0.0, 0, 3, 1, idx, comb, mg)
    assert all_finite(comb) and all_finite(mg) and fence_intact(cbuf) and fence_intact(mbuf)
    assert bool((ibuf[:FENCE] == -1).all()) and bool((ibuf[-FENCE:] == -1).all()) and int(idx.min()) >= 0 and int(idx.max()) < V
    flat, cflat = logits.view(2 * B * l, V), comb.view(B * l, V)
    windows = op_windows('cfg_sample')
    refs = {}
    for lo, hi in windows:
        ref = (1 + t) * flat[lo:hi].cpu() - t * flat[B * l + lo:B * l + hi].cpu()
        refs[lo] = ref
        assert torch.equal(cflat[lo:hi].cpu(), ref), (lo, hi)                                    # same evaluation order -> bit identical
        assert torch.equal(idx.view(-1)[lo:hi].cpu().long(), ref.argmax(-1)), (lo, hi)
        t2 = ref.topk(2, dim=-1).values
        assert torch.allclose(mg.view(-1)[lo:hi].cpu(), t2[..., 0] - t2[..., 1]), (lo, hi)
    nb = B // NCHUNK
    for b0 in range(0, B, nb):
        small_lg = torch.cat((logits[b0:b0 + nb], logits[B + b0:B + b0 + nb]))
        sc = torch.full((nb, l, V), float('nan'), device=dev)
        si = torch.full((nb, l), -1, dtype=torch.int32, device=dev)
        sm = torch.full((nb, l), float('nan'), device=dev)
        ops.cfg_sample(small_lg, nb, 2, l, V, coef, 1, 0.0, 0, 3, 1, si, sc, sm)
        assert failing_chunks(comb[b0:b0 + nb], [(0, nb, sc)], nb) == [], b0
        assert torch.equal(idx[b0:b0 + nb], si) and torch.equal(mg[b0:b0 + nb], sm), b0
        del small_lg, sc, si, sm
    # ---- the reference's sampling defaults, on the window rows
    k, p = 900, 0.96
    kept = torch.full((B, l), -1, dtype=torch.int32, device=dev)
    idx.fill_(-1)
    ops.cfg_sample(logits, B, 2, l, V, coef, k, p, 1234, 2, 1, idx, None, None, kept)
    assert int(idx.min()) >= 0 and int(idx.max()) < V and int(kept.min()) >= 1
    assert bool((ibuf[:FENCE] == -1).all()) and bool((ibuf[-FENCE:] == -1).all())
    for lo, hi in windows:
        ref = refs[lo]
        masked = topk_topp_mask_(ref.clone(), k, p)
        kept_ref = torch.isfinite(masked)
        i = idx.view(-1)[lo:hi].cpu().long()
        assert kept_ref.gather(-1, i.unsqueeze(-1)).all(), ('draw outside the reference kept set', lo, hi)
        dk = kept.view(-1)[lo:hi].cpu().long() - kept_ref.sum(-1)
        assert dk.abs().max() <= 1, (lo, hi)
        if dk.abs().max() > 0:            # one token either way only where the nucleus threshold falls within fp32 rounding of a cumulative probability
            cs = ref.double().sort(-1, descending=False)[0].softmax(-1).cumsum(-1)
            n_rm = V - kept_ref.sum(-1)
            for (r_,) in torch.nonzero(dk):
                near = cs[r_, max(int(n_rm[r_]) - 1, 0):int(n_rm[r_]) + 1]
                assert ((near - (1 - p)).abs() < 1e-5).any(), f'kept-set differs away from the threshold: {near.tolist()} vs {1 - p}'
    del logits, cbuf, comb, ibuf, idx, mbuf, mg, kept, refs
    release()


@pytest.mark.gpu
def test_word_embed_writes_the_headline_stream(gpu_device):
    """cvar_word_embed: tokens (512, 512, 32) -> the (1024 x 512, 1536) fp32 stream, both CFG copies (nrep = 2), level rows 848.. of the position table.
    Bound: 1e-5 absolute (test_word_embed_first_tokens).  Peak: x 3.2 GB + one chunk 0.4 GB = 3.6 GB."""
    dev = gpu_device
    need(dev, 5 << 30)
    nb, l, Cv = B_HEAD, L_LAST, CFG24.cvae
    g = torch.Generator(device=dev).manual_seed(111)
    tok = dev_randn((nb, l, Cv), F32, dev, g)
    # W ~ N(0, 1 / Cvae): outputs of O(1) like the trained embedding's - the absolute 1e-5 of the small test is an fp32 bound for values of that size
    # (unit-variance W gives |x| up to 30, where 34 chained fp32 roundings reach 1.2e-5: measured on the first window, not an addressing error)
    W, bias, lvl = dev_randn((C, Cv), F32, dev, g, std=Cv ** -0.5), dev_randn((C,), F32, dev, g), dev_randn((LMAX, C), F32, dev, g)
    buf, x = fenced((2 * nb * l, C), F32, dev)
    ops.word_embed(tok, W, bias, lvl, x, nb, 2, l, Cv, C, l, 0, lvl_off=Q_OFF)
    Wd, bd, lv = host64(W), host64(bias), host64(lvl[Q_OFF:Q_OFF + l])
    tflat = tok.view(nb * l, Cv)

    def reference(lo, hi):
        rows = torch.arange(lo, hi) % (nb * l)                                # row of the token tensor: the second copy repeats the first
        t0, t1 = int(rows.min()), int(rows.max()) + 1
        return host64(tflat[t0:t1])[rows - t0] @ Wd.t() + bd + lv[rows % l]

    def accept(got, ref):
        err = float((got.double() - ref).abs().max())
        print(f'word_embed window: max |x - float64| = {err:.2e}')
        return err < 1e-5

    bad = failing_windows(lambda lo, hi: x[lo:hi].cpu(), reference, op_windows('word_embed'), accept)
    assert bad == [], bad
    nbc = nb // NCHUNK
    for b0 in range(0, nb, nbc):
        small = torch.full((2 * nbc * l, C), float('nan'), device=dev)
        ops.word_embed(tok[b0:b0 + nbc], W, bias, lvl, small, nbc, 2, l, Cv, C, l, 0, lvl_off=Q_OFF)
        for rep in range(2):
            big = x[(rep * nb + b0) * l:(rep * nb + b0 + nbc) * l]
            assert failing_chunks(big, [(0, nbc * l, small[rep * nbc * l:(rep + 1) * nbc * l])], nbc * l) == [], (b0, rep)
        del small
    assert fence_intact(buf)
    del tok, buf, x
    release()


@pytest.mark.gpu
def test_images_decode_and_encode_to_the_same_bits_in_a_batch_of_128(gpu_device):
    """test_an_image_decodes_and_encodes_to_the_same_bits_in_any_batch at the decode chunk of generation (128 images, ch 160, bf16): the (128 x 65536, 160)
    activations cross 2^31 bytes inside image 102.  Images 0, 101, 102, 103, 127 of the batch against the same five on their own, bit for bit.
    Peak: a few (128 x 65536, 160) bf16 activations of 2.7 GB each and their fp32 outputs: below 20 GB."""
    from test_gpu_parity import make_vae
    from controlvar_amd.synth import synth_images
    dev = gpu_device
    need(dev, 30 << 30)
    vae = make_vae(DEC_CH, BF16, dev)
    assert vae.decode_chunk == DECODE_CHUNK
    picks = list(VAE_PICKS)
    g = torch.Generator().manual_seed(11)
    f_hat = (torch.randn(DECODE_CHUNK, 32, 16, 16, generator=g) * 0.7).to(dev)
    with torch.no_grad():
        big = vae.fhat_to_img(f_hat)
        small = vae.fhat_to_img(f_hat[picks].contiguous())
    assert torch.isfinite(big).all()
    for j, i in enumerate(picks):
        assert torch.equal(big[i], small[j]), ('decode', i, float((big[i] - small[j]).abs().max()))
    del big, small
    release()
    img = synth_images(DECODE_CHUNK, 256, seed=5).to(dev)
    with torch.no_grad():
        fb = vae._encode_f(img)
        fs = vae._encode_f(img[picks].contiguous())
    assert torch.isfinite(fb).all()
    for j, i in enumerate(picks):
        assert torch.equal(fb[i], fs[j]), ('encode', i, float((fb[i] - fs[j]).abs().max()))
    del vae, img, fb, fs, f_hat
    release()


# ------------------------------------------------------------------------------------------------ Part 2: a whole generation at B = 512
def _gen(m, B, labels, types, force=None):
    img = m.autoregressive_infer_cfg(B, labels, g_seed=5, cfg=4.0, top_k=1, cond_type=types, _trace=True, **({'_force_idx': force} if force is not None else {}))
    return img, m.last_trace


@pytest.mark.gpu
def test_generation_at_batch_512_with_512_different_rows(gpu_device):
    """A depth-2 ControlVAR of d24 width (C = 1536, 24 heads, hidden 6144, V = 4096, ch-160 VQVAE, bf16) generates 512 DIFFERENT (label, condition type)
    samples at once - the row counts and kernels of the headline, an arena of two layers - and samples {0, 1, 2, 3, 255, 256, 511} again as a batch of 7.
    deterministic_plan: ids, per-scale CFG logits and images of those rows bit-identical (models.ControlVAR: "at any batch size").  Default plan: the batch
    of 7 forced along the ids of the 512, logits within BF16_REL_BOUND and greedy ids equal wherever the margin exceeds it, as
    test_one_sample_across_batch_sizes_and_gemm_plans; the ids being forced, the images are the same bits.
    Peak: arena 17.1 GB + per pass x 3.2, u / o / q 4.8, hbuf 6.4, logits 8.6 GB + trace (512, 1360, 4096) fp32 11.4 GB + decode chunk ~10 GB: ~60 GB."""
    from test_gpu_configs import BF16_REL_BOUND
    from test_gpu_parity import make_vae, make_var
    dev = gpu_device
    need(dev, 80 << 30)
    B = B_HEAD
    cfg = VarConfig(depth=2, embed_dim=C, num_heads=H)
    vae = make_vae(DEC_CH, BF16, dev)
    m = make_var(vae, cfg, BF16, dev)
    labels = (torch.arange(B) * 37 + 11) % 1000
    types = torch.arange(B) % 4
    assert len({(int(a), int(b)) for a, b in zip(labels, types)}) == B and labels.unique().numel() == B
    picks = list(GEN_PICKS)

    def keep(img, tr, rows):
        return [x[rows].clone() for x in tr['idx']], [x[rows].float().clone() for x in tr['logits']], img[rows].clone()

    try:
        m.deterministic_plan = True
        img, tr = _gen(m, B, labels, types)
        assert img.shape == (B, 3, 512, 256) and bool(torch.isfinite(img).all())
        ids_b, lg_b, img_b = keep(img, tr, picks)
        # the rows really differ: a row that read its neighbour's memory would not reproduce its own sample below
        for a in range(len(picks)):
            for b in range(a + 1, len(picks)):
                assert not torch.equal(lg_b[0][a], lg_b[0][b]) and not torch.equal(img_b[a], img_b[b]), (picks[a], picks[b])
        del img, tr
        m.last_trace = None
        release()
        img, tr = _gen(m, len(picks), labels[picks], types[picks])
        ids_s, lg_s, img_s = keep(img, tr, list(range(len(picks))))
        for si in range(len(PN)):
            assert torch.equal(ids_b[si], ids_s[si]), ('ids', si, int((ids_b[si] != ids_s[si]).sum()))
            assert torch.equal(lg_b[si], lg_s[si]), ('logits', si, float((lg_b[si] - lg_s[si]).abs().max()))
        for j, s in enumerate(picks):
            assert torch.equal(img_b[j], img_s[j]), ('image', s, float((img_b[j] - img_s[j]).abs().max()))
        del img, tr, ids_b, lg_b, img_b, ids_s, lg_s, img_s
        m.last_trace = None
        release()

        m.deterministic_plan = False
        img, tr = _gen(m, B, labels, types)
        ids_b, lg_b, img_b = keep(img, tr, picks)
        del img, tr
        m.last_trace = None
        release()
        img, tr = _gen(m, len(picks), labels[picks], types[picks], force=[i.long() for i in ids_b])
        ids_s, lg_s, img_s = keep(img, tr, list(range(len(picks))))
        worst, flips = 0.0, 0
        for si in range(len(PN)):
            a, b = lg_s[si], lg_b[si]
            amax = float(b.abs().max())
            d = float((a - b).abs().max()) / amax
            worst = max(worst, d)
            assert d <= BF16_REL_BOUND, (si, d)
            t2 = b.topk(2, dim=-1).values
            margin = t2[..., 0] - t2[..., 1]
            mism = a.argmax(-1) != b.argmax(-1)
            flips += int(mism.sum())
            assert not bool((mism & (margin > BF16_REL_BOUND * amax)).any()), si
        print(f'[bf16] 7 of 512 samples, default plan, B = 7 forced along the B = 512 ids: largest logit distance {worst:.2e} of max|logit|, {flips} argmax flips')
        for j, s in enumerate(picks):
            assert torch.equal(img_b[j], img_s[j]), ('image', s, float((img_b[j] - img_s[j]).abs().max()))
    finally:
        m.deterministic_plan = False
        m.last_trace = None
        m._arena = None
    del m, vae
    release()
