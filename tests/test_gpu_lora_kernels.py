"""The cvar_lora_* kernels (csrc/lora.hip) op by op against float64 references built from the host copy of the dropout mask
(oracle/lora_ref.py):

* the mask itself, bit for bit;
* exact integer cases: inputs in [-2, 2], p in {0, 0.5, 0.75} (1 / (1 - p) = 1, 2, 4) and scale 1 or 2 keep every product and partial
  sum an integer below 2^24, so the accumulation order cannot matter.  fp32 outputs must equal the float64 reference exactly, bf16
  outputs the reference rounded to bf16 (RNE) exactly - a dropped row at a slab or split boundary, a mask on the wrong element or a
  missing scale changes an integer;
* random-value cases with rounding bounds, the fused GELU' of cvar_lora_dx, and the <bf16 du, fp32 dx> pair;
* fences: every operand lives in a NaN-filled arena, and every byte outside the declared outputs must be unchanged;
* the three calling forms of the training engine, and rejected arguments."""
import numpy as np
import pytest
import torch

from controlvar_amd import ops
from controlvar_amd._lib import CvarError
from oracle import lora_ref, var_ref

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24                      # fp32 unit roundoff
SEEDS = [2 ** 33 + 5, -3, 7, 2 ** 63 + 11]


def cdiv(a, b):
    return -(-a // b)


def arena(rows, ld, dtype, dev, pad=64, fill=float('nan')):
    """(flat buffer, rows x ld window at element offset pad): pad elements of `fill` before and after, 16-byte aligned"""
    buf = torch.full((2 * pad + rows * ld,), fill, dtype=dtype, device=dev)
    return buf, buf[pad:pad + rows * ld].view(rows, ld)


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def ints(shape, gen, dtype, dev):
    return torch.randint(-2, 3, shape, generator=gen).to(dtype).to(dev)


def factor(M, K, p, seed, tag, dev):
    """(M, K) float64 inverted-dropout factor from the host mask"""
    if p == 0:
        return torch.ones(M, K, dtype=torch.float64, device=dev)
    keep = torch.from_numpy(lora_ref.keep_mask(M, K, p, seed, tag)).to(dev)
    return torch.where(keep, lora_ref.inv_keep(p), 0.0).to(torch.float64)


def wgrad_splits(M, N):
    """csrc/lora.hip wgrad_plan: the number of M slices"""
    ns = max(1, min(cdiv(1024, cdiv(N, 512)), cdiv(M, 64)))
    rps = cdiv(cdiv(M, ns), 64) * 64
    return cdiv(M, rps)


def rounded(ref, dtype):
    """what an exact kernel stores: the float64 reference rounded once (it is an integer below 2^24, so float32 holds it exactly)"""
    assert (ref.abs() < 2 ** 24).all() and torch.equal(ref, ref.round())
    return ref.to(F32).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- the mask
@pytest.mark.parametrize('p', [1e-9, 0.05, 0.3, 0.5, 0.999])
def test_device_mask_equals_the_host_copy(gpu_device, p):
    for (M, K), seed, tag in (((1, 1), 0, 0), ((3, 1000), 2 ** 32 + 5, 5), ((257, 511), -1, 99), ((1003, 333), 2 ** 63 + 11, 2 ** 31 + 3),
                              ((64, 6144), -12345, 4 * 24 + 3), ((2, 9216), 7, 95)):
        got = ops.lora_dropout_mask(M, K, p, seed, tag, device=gpu_device).cpu().numpy()
        want = lora_ref.keep_mask(M, K, p, seed, tag)
        assert np.array_equal(got, want.astype(np.float32)), (M, K, p, seed, tag, int((got != want).sum()))
    assert torch.equal(ops.lora_dropout_mask(5, 24, 0.0, 1, 1, device=gpu_device), torch.ones(5, 24, device=gpu_device))


# ---------------------------------------------------------------------------------------------------------------- exact: down
DOWN = [  # M, K, r, dtype, p, scale
    (1, 8, 1, F32, 0.5, 2.0),
    (15, 504, 5, BF16, 0.75, 1.0),
    (16, 512, 16, F32, 0.0, 2.0),
    (17, 520, 15, BF16, 0.5, 2.0),
    (1003, 1000, 16, F32, 0.75, 2.0),
    (1003, 1536, 5, BF16, 0.5, 1.0),
    (4099, 6144, 16, BF16, 0.5, 2.0),
    (64, 6144, 1, F32, 0.75, 1.0),
    (43520, 1536, 16, BF16, 0.5, 2.0),
    (43520, 6144, 16, F32, 0.0, 2.0),
]


@pytest.mark.parametrize('M,K,r,dtype,p,scale', DOWN)
def test_down_exact_inside_nan_arenas(gpu_device, M, K, r, dtype, p, scale):
    dev = gpu_device
    g = torch.Generator().manual_seed(M * 7 + K + r)
    seed, tag = SEEDS[(M + K) % 4], (M + r) % 100
    ldx, lda, ldu = K + 8 * (M % 3), K + 16, r + (M % 5)
    xb, x = arena(M, ldx, dtype, dev)
    x[:, :K] = ints((M, K), g, dtype, dev)
    ab, A = arena(r, lda, dtype, dev)
    A[:, :K] = ints((r, K), g, dtype, dev)
    ub, u = arena(M, ldu, dtype, dev)
    cb, xc = arena(M, K, dtype, dev)
    x0, a0 = xb.clone(), ab.clone()
    ops.lora_down(x, A, u, M=M, K=K, r=r, scale=scale, p=p, seed=seed, tag=tag, ldx=ldx, lda=lda, ldu=ldu, x_copy=xc if p > 0 else None)
    ref = scale * (x[:, :K].double() * factor(M, K, p, seed, tag, dev)) @ A[:, :K].double().t()
    want = ub.clone()
    want[64:64 + M * ldu].view(M, ldu)[:, :r] = rounded(ref, dtype)
    assert same_bits(ub, want), (ub[64:64 + M * ldu].view(M, ldu)[:, :r].double() - ref).abs().max().item()
    assert same_bits(xb, x0) and same_bits(ab, a0)                     # inputs untouched
    if p > 0:                                                            # x_copy: x before dropout, nothing else written
        wantc = torch.full_like(cb, float('nan'))
        wantc[64:64 + M * K] = x[:, :K].reshape(-1)
        assert same_bits(cb, wantc)


# ---------------------------------------------------------------------------------------------------------------- exact: dx
DX = [  # M, K, r, du dtype, dx dtype, p, scale
    (1, 8, 16, F32, F32, 0.75, 2.0),
    (15, 504, 1, BF16, BF16, 0.5, 2.0),
    (16, 512, 5, BF16, F32, 0.5, 1.0),
    (17, 520, 16, F32, F32, 0.0, 1.0),
    (1003, 1000, 15, BF16, BF16, 0.75, 2.0),
    (1003, 6144, 5, F32, F32, 0.5, 2.0),
    (43520, 1536, 16, BF16, F32, 0.5, 2.0),
    (43520, 1536, 5, BF16, BF16, 0.75, 2.0),
]


@pytest.mark.parametrize('M,K,r,dtype,dxt,p,scale', DX)
def test_dx_exact_inside_nan_arenas(gpu_device, M, K, r, dtype, dxt, p, scale):
    dev = gpu_device
    g = torch.Generator().manual_seed(M * 5 + K + r)
    seed, tag = SEEDS[(M + r) % 4], (K + r) % 100
    lddx, lddu, lda = K + 8 * (M % 2), 16 + 8 * (K % 2 == 0 and M % 3 == 0), K + 8
    db, dx = arena(M, lddx, dxt, dev)
    dx[:, :K] = ints((M, K), g, dxt, dev)
    ub, du = arena(M, lddu, dtype, dev)                                  # du columns >= r stay NaN: the kernel must ignore them
    du[:, :r] = ints((M, r), g, dtype, dev)
    ab, A = arena(r, lda, dtype, dev)                                    # rows >= r of A do not exist
    A[:, :K] = ints((r, K), g, dtype, dev)
    dx0 = dx[:, :K].double()
    u0, a0 = ub.clone(), ab.clone()
    ops.lora_dx(dx, du, A, M=M, K=K, r=r, scale=scale, p=p, seed=seed, tag=tag, lddx=lddx, lddu=lddu, lda=lda)
    ref = dx0 + scale * factor(M, K, p, seed, tag, dev) * (du[:, :r].double() @ A[:, :K].double())
    want = torch.full_like(db, float('nan'))
    want[64:64 + M * lddx].view(M, lddx)[:, :K] = rounded(ref, dxt)
    assert same_bits(db, want), (dx[:, :K].double() - ref).abs().max().item()
    assert same_bits(ub, u0) and same_bits(ab, a0)


# ---------------------------------------------------------------------------------------------------------------- exact: wgrad
WG = [  # M, N, r, dtype, p, scale, transposed output, splits
    (2, 2, 16, F32, 0.5, 2.0, False, 1),
    (64, 192, 5, BF16, 0.75, 1.0, True, 1),
    (1003, 9216, 16, BF16, 0.5, 2.0, False, 16),
    (1003, 192, 1, F32, 0.0, 1.0, True, 16),
    (43520, 6144, 16, BF16, 0.0, 1.0, False, 85),
    (43520, 6144, 16, F32, 0.75, 2.0, True, 85),
    (43520, 1536, 5, BF16, 0.5, 2.0, True, 340),
    (43520, 1536, 15, F32, 0.0, 1.0, False, 340),
    (43520, 2, 16, BF16, 0.5, 2.0, False, 680),
]


@pytest.mark.parametrize('M,N,r,dtype,p,scale,tr,splits', WG)
def test_wgrad_exact_with_a_nan_workspace(gpu_device, M, N, r, dtype, p, scale, tr, splits):
    dev = gpu_device
    assert wgrad_splits(M, N) == splits and ops.lora_wgrad_ws_floats(M, N) == splits * N * 16
    g = torch.Generator().manual_seed(M + N * 3 + r)
    seed, tag = SEEDS[(N + r) % 4], (M + N) % 100
    ldy, ldz = N + 2 * (M % 3), r + 3
    yb, Y = arena(M, ldy, dtype, dev)
    Y[:, :N] = ints((M, N), g, dtype, dev)
    zb, Z = arena(M, ldz, dtype, dev)
    Z[:, :r] = ints((M, r), g, dtype, dev)
    nws = ops.lora_wgrad_ws_floats(M, N)
    wsb = torch.full((nws + 128,), float('nan'), device=dev)
    off = 12
    if tr:                                                               # the engine's dA layout: out[j * N + n]
        os_n, os_j, size = 1, N, r * N
    else:                                                                # [N][r] with a gap of 3 between rows
        os_n, os_j, size = r + 3, 1, N * (r + 3)
    ob = torch.full((off + size + 64,), float('nan'), device=dev)
    y0, z0 = yb.clone(), zb.clone()
    ops.lora_wgrad(Y, Z, ob, wsb[:nws], M=M, N=N, r=r, scale=scale, p=p, seed=seed, tag=tag, ldy=ldy, ldz=ldz, out_off=off, os_n=os_n, os_j=os_j)
    ref = scale * (Y[:, :N].double() * factor(M, N, p, seed, tag, dev)).t() @ Z[:, :r].double()          # (N, r)
    want = torch.full_like(ob, float('nan'))
    n_idx = torch.arange(N, device=dev)[:, None]
    j_idx = torch.arange(r, device=dev)[None, :]
    want[off + n_idx * os_n + j_idx * os_j] = rounded(ref, F32)
    assert same_bits(ob, want)
    assert torch.isnan(wsb[nws:]).all()                                 # nothing past the declared workspace
    assert same_bits(yb, y0) and same_bits(zb, z0)


def test_wgrad_is_bit_identical_from_run_to_run(gpu_device):
    dev = gpu_device
    g = torch.Generator().manual_seed(4)
    M, N, r = 43520, 1536, 16
    Y, Z = torch.randn(M, N, generator=g).to(BF16).to(dev), torch.randn(M, r, generator=g).to(BF16).to(dev)
    ws = torch.empty(ops.lora_wgrad_ws_floats(M, N), device=dev)
    outs = []
    for fill in (float('nan'), 0.0):                                     # what the workspace held before does not matter
        ws.fill_(fill)
        out = torch.empty(N, r, device=dev)
        outs.append(ops.lora_wgrad(Y, Z, out, ws, M=M, N=N, r=r, scale=2.0, p=0.05, seed=9, tag=3))
    assert same_bits(outs[0], outs[1])
    ref = 2.0 * (Y.double() * factor(M, N, 0.05, 9, 3, dev)).t() @ Z.double()
    S = 2.0 * (Y.double().abs() * factor(M, N, 0.05, 9, 3, dev)).t() @ Z.double().abs()
    assert ((outs[0].double() - ref).abs() <= (M + 8) * U * S + 1e-30).all()                  # any fp32 summation order of M terms


# ---------------------------------------------------------------------------------------------------------------- random values
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_down_random_values_with_rounding_bounds(gpu_device, dtype):
    dev = gpu_device
    g = torch.Generator().manual_seed(1)
    M, K, r, s, p, seed, tag = 2720, 1000, 16, 2.0, 0.05, 2 ** 40 + 1, 6
    x = torch.randn(M, K, generator=g).to(dtype).to(dev)
    x[0, :4] = torch.tensor([-0.0, 1e-40, 3e38, -1e-30]).to(dtype).to(dev)        # signed zero, a denormal, a huge value: copied as they are
    A = ((torch.rand(r, K, generator=g) * 2 - 1) / K ** 0.5).to(dtype).to(dev)
    u = torch.empty(M, r, device=dev, dtype=dtype)
    xc = torch.empty(M, K, device=dev, dtype=dtype)
    ops.lora_down(x, A, u, M=M, K=K, r=r, scale=s, p=p, seed=seed, tag=tag, x_copy=xc)
    assert same_bits(xc, x)
    f = factor(M, K, p, seed, tag, dev)
    ref = s * (x.double() * f) @ A.double().t()
    S = s * (x.double().abs() * f) @ A.double().abs().t()
    bound = (K + 2) * U * S                                              # fp32 dot product of K terms, one fp32 product by 1/(1-p), the scale
    if dtype == BF16:
        bound = bound + ref.abs() * 2.0 ** -8                            # one bf16 rounding of the output (half an ulp is 2^-9 relative)
    assert ((u.double() - ref).abs() <= bound + 1e-30).all()


@pytest.mark.parametrize('dtype,dxt', [(F32, F32), (BF16, BF16), (BF16, F32)])
def test_dx_with_fused_gelu_grad(gpu_device, dtype, dxt):
    dev = gpu_device
    g = torch.Generator().manual_seed(2)
    M, K, r, s, p, seed, tag = 1003, 1536, 5, 6.4, 0.3, -77, 2
    dx = torch.randn(M, K, generator=g).to(dxt).to(dev)
    du = torch.randn(M, 16, generator=g).to(dtype).to(dev)
    A = (torch.randn(r, K, generator=g) / 8).to(dtype).to(dev)
    aux = (torch.randn(M, K, generator=g) * 3).to(dtype).to(dev)
    dx0 = dx.double()
    ops.lora_dx(dx, du, A, M=M, K=K, r=r, scale=s, p=p, seed=seed, tag=tag, aux=aux)
    f = factor(M, K, p, seed, tag, dev)
    t = aux.double().requires_grad_(True)
    var_ref.gelu_tanh(t).sum().backward()
    gp = t.grad                                                          # d gelu_tanh / dt in float64
    pre = dx0 + s * f * (du[:, :r].double() @ A.double())
    S = dx0.abs() + s * f * (du[:, :r].double().abs() @ A.double().abs())
    # fp32: r-term dot product, the product by s * keep, the add (r + 3 roundings of S), times gelu' computed in fp32 with a fast exp
    # (absolute error below 1e-5 on a value of at most 1.13), and the final product
    bound = (r + 4) * U * S * gp.abs() + 1e-5 * pre.abs()
    if dxt == BF16:
        bound = bound + (pre * gp).abs() * 2.0 ** -8
    err = (dx.double() - pre * gp).abs()
    assert (err <= bound + 1e-30).all(), (err - bound).max().item()


# ---------------------------------------------------------------------------------------------------------------- the engine's forms
@pytest.mark.parametrize('dtype,r', [(BF16, 16), (F32, 5)])
def test_engine_forms_of_the_block_targets(gpu_device, dtype, r):
    """proj / fc1: x_copy into [x | u | 0] with u at column K; fc2: x and u in one buffer (ldx = ldu = hid + rp, u_off = hid).  The
    padding columns [K + r, K + rp) must stay zero - K-augmentation multiplies them with the zero columns of [W | B | 0]."""
    dev = gpu_device
    g = torch.Generator().manual_seed(3)
    M, C, rp, s, p, seed = 2720, 320, 128 // (2 if dtype == BF16 else 4), 2.0, 0.5, 2 ** 35 + 3
    hid = 4 * C
    kc, kh = C + rp, hid + rp
    x = ints((M, C), g, dtype, dev)
    A = torch.zeros(16, C, device=dev, dtype=dtype)
    A[:r] = ints((r, C), g, dtype, dev)
    xa = torch.zeros(M, kc, device=dev, dtype=dtype)
    ops.lora_down(x, A, xa, M=M, K=C, r=r, scale=s, p=p, seed=seed, tag=4, ldu=kc, u_off=C, x_copy=xa, ld_copy=kc)
    assert same_bits(xa[:, :C], x)
    assert torch.equal(xa[:, C:C + r], rounded(s * (x.double() * factor(M, C, p, seed, 4, dev)) @ A[:r].double().t(), dtype))
    assert same_bits(xa[:, C + r:], torch.zeros(M, kc - C - r, device=dev, dtype=dtype))
    # fc2: in place
    H = torch.zeros(M, kh, device=dev, dtype=dtype)
    H[:, :hid] = ints((M, hid), g, dtype, dev)
    A2 = torch.zeros(16, hid, device=dev, dtype=dtype)
    A2[:r] = ints((r, hid), g, dtype, dev)
    h0 = H[:, :hid].clone()
    ops.lora_down(H, A2, H, M=M, K=hid, r=r, scale=s, p=p, seed=seed, tag=6, ldx=kh, ldu=kh, u_off=hid)
    assert same_bits(H[:, :hid], h0)
    assert torch.equal(H[:, hid:hid + r], rounded(s * (h0.double() * factor(M, hid, p, seed, 6, dev)) @ A2[:r].double().t(), dtype))
    assert same_bits(H[:, hid + r:], torch.zeros(M, kh - hid - r, device=dev, dtype=dtype))
    # the backward reads u and x back out of the augmented rows: dB = dY^T u (p = 0), dA = s du^T drop(x) (engine's transposed layout)
    dY = ints((M, C), g, dtype, dev)
    du = torch.full((M, 16), float('nan'), device=dev, dtype=dtype)
    du[:, :r] = ints((M, r), g, dtype, dev)
    G = torch.full((7 + C * r + hid * r,), float('nan'), device=dev)
    ws = torch.empty(max(ops.lora_wgrad_ws_floats(M, C), ops.lora_wgrad_ws_floats(M, hid)), device=dev)
    H[:, hid:hid + r] = ints((M, r), g, dtype, dev)                      # small u: dB stays an exact integer
    ops.lora_wgrad(dY, H, G, ws, M=M, N=C, r=r, ldz=kh, z_off=hid, out_off=7)
    ops.lora_wgrad(H, du, G, ws, M=M, N=hid, r=r, scale=s, p=p, seed=seed, tag=6, ldy=kh, ldz=16, out_off=7 + C * r, os_n=1, os_j=hid)
    dB = dY.double().t() @ H[:, hid:hid + r].double()
    dA = s * du[:, :r].double().t() @ (h0.double() * factor(M, hid, p, seed, 6, dev))
    assert torch.equal(G[7:7 + C * r].view(C, r), rounded(dB, F32))
    assert torch.equal(G[7 + C * r:].view(r, hid), rounded(dA, F32))
    assert torch.isnan(G[:7]).all()


@pytest.mark.parametrize('dtype,r', [(BF16, 16), (F32, 5)])
def test_engine_forms_of_the_adaln_targets(gpu_device, dtype, r):
    """forward: u_t at the columns C + 16 t of [cs | u_0 ... u_depth] (x_copy with the first); backward: du_t = dada[:, t 6C : ...] B_t
    (x_off = t 6C, lda = 6C, the head's K = 2C) and the B / A gradients with y_off = t 6C, ldy = n_ada and z_off = C + 16 t"""
    dev = gpu_device
    g = torch.Generator().manual_seed(4)
    B, C, depth, s, p, seed = 3, 320, 2, 2.0, 0.75, -5
    rp = 128 // (2 if dtype == BF16 else 4)
    Kx = cdiv((depth + 1) * 16, rp) * rp
    ld, n_ada = C + Kx, depth * 6 * C + 2 * C
    cs = ints((B, C), g, dtype, dev)
    LA = torch.zeros(depth + 1, 16, C, device=dev, dtype=dtype)
    LA[:, :r] = ints((depth + 1, r, C), g, dtype, dev)
    csa = torch.zeros(B, ld, device=dev, dtype=dtype)
    for t in range(depth + 1):
        ops.lora_down(cs, LA[t], csa, M=B, K=C, r=r, scale=s, p=p, seed=seed, tag=4 * t + 3, ldu=ld, u_off=C + 16 * t,
                      x_copy=csa if t == 0 else None, ld_copy=ld)
    want = torch.zeros(B, ld, device=dev, dtype=dtype)
    want[:, :C] = cs
    for t in range(depth + 1):
        want[:, C + 16 * t:C + 16 * t + r] = rounded(s * (cs.double() * factor(B, C, p, seed, 4 * t + 3, dev)) @ LA[t, :r].double().t(), dtype)
    assert same_bits(csa, want)
    dada = ints((B, n_ada), g, dtype, dev)
    LBT = torch.full((depth + 1, 16, 6 * C), float('nan'), device=dev, dtype=dtype)
    for t in range(depth + 1):
        n_out = 6 * C if t < depth else 2 * C
        LBT[t, :r, :n_out] = ints((r, n_out), g, dtype, dev)
        du = torch.full((B, 16), float('nan'), device=dev, dtype=dtype)
        ops.lora_down(dada, LBT[t], du, M=B, K=n_out, r=r, scale=1.0, ldx=n_ada, x_off=t * 6 * C, lda=6 * C, ldu=16)
        y = dada[:, t * 6 * C:t * 6 * C + n_out].double()
        assert torch.equal(du[:, :r], rounded(y @ LBT[t, :r, :n_out].double().t(), dtype))
        assert torch.isnan(du[:, r:]).all()
        G = torch.full((n_out * r + r * C,), float('nan'), device=dev)
        ws = torch.empty(max(ops.lora_wgrad_ws_floats(B, n_out), ops.lora_wgrad_ws_floats(B, C)), device=dev)
        ops.lora_wgrad(dada, csa, G, ws, M=B, N=n_out, r=r, ldy=n_ada, y_off=t * 6 * C, ldz=ld, z_off=C + 16 * t)
        ops.lora_wgrad(csa, du, G, ws, M=B, N=C, r=r, scale=s, p=p, seed=seed, tag=4 * t + 3, ldy=ld, ldz=16, out_off=n_out * r, os_n=1, os_j=C)
        assert torch.equal(G[:n_out * r].view(n_out, r), rounded(y.t() @ csa[:, C + 16 * t:C + 16 * t + r].double(), F32))
        dA = s * du[:, :r].double().t() @ (cs.double() * factor(B, C, p, seed, 4 * t + 3, dev))
        assert torch.equal(G[n_out * r:].view(r, C), rounded(dA, F32))


def test_lora_randomised_sweep_inside_nan_arenas(gpu_device):
    """60 random down / dx / wgrad problems (shapes, strides, offsets, ranks, rates, seeds, dtype pairs, in-place forms) inside NaN
    arenas against float64 (tools/fuzz_lora.py is the same sweep at any size)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'fuzz_lora.py'), '60', '3'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '60/60 cases ok' in r.stdout


# ---------------------------------------------------------------------------------------------------------------- rejected arguments
def test_rejected_arguments_leave_the_device_usable(gpu_device):
    dev = gpu_device
    x = torch.ones(64, 64, device=dev)
    A = torch.ones(16, 64, device=dev)
    u = torch.zeros(64, 16, device=dev)
    ws = torch.empty(ops.lora_wgrad_ws_floats(64, 64), device=dev)
    out = torch.zeros(64, 16, device=dev)
    down = dict(M=64, K=64, r=16, scale=1.0, ldu=16)
    with pytest.raises(CvarError):
        ops.lora_down(x, A, u, **{**down, 'r': 0})                                        # r = 0
    with pytest.raises(CvarError):
        ops.lora_down(x, A, u, **{**down, 'r': 17})                                       # r above the register rank 16
    with pytest.raises(CvarError):
        ops.lora_down(x, A, u, **{**down, 'K': 60})                                       # K % 8
    with pytest.raises(CvarError):
        ops.lora_down(x, A, u, **down, ldx=56)                                            # ldx < K
    with pytest.raises(CvarError):
        ops.lora_down(x, A, u, **down, x_off=1)                                           # x not 16-byte aligned
    with pytest.raises(CvarError):
        ops.lora_down(x, A, u, **down, p=1.0)                                             # p = 1
    with pytest.raises(CvarError):
        ops.lora_down(x, A, u, **down, p=-0.1)                                            # p < 0
    with pytest.raises(CvarError):
        ops.lora_dx(x, u, A, M=64, K=64, r=16, scale=1.0, p=1.0)                          # p = 1
    with pytest.raises(CvarError):
        ops.lora_dx(x, u, A, M=64, K=64, r=0, scale=1.0)                                  # r = 0
    with pytest.raises(CvarError):
        ops.lora_dx(x, u, A, M=64, K=64, r=16, scale=1.0, lddu=8)                         # du rows narrower than 16
    with pytest.raises(CvarError):
        ops.lora_dx(x.to(BF16), u, A, M=64, K=64, r=16, scale=1.0)                        # bf16 dx with fp32 du: no such pair
    with pytest.raises(TypeError):
        ops.lora_down(x, A.to(BF16), u, **down)                                           # operand dtypes differ
    with pytest.raises(TypeError):
        ops.lora_down(x.half(), A.half(), u.half(), **down)                               # fp16 is not a compute dtype
    with pytest.raises(CvarError):
        ops.lora_wgrad(x, u, out, ws[:-1], M=64, N=64, r=16)                              # workspace too small
    with pytest.raises(CvarError):
        ops.lora_wgrad(x, u, out, ws, M=64, N=63, r=16)                                   # odd N
    with pytest.raises(CvarError):
        ops.lora_wgrad(x, u, out, ws, M=64, N=64, r=17)                                   # r = 17
    with pytest.raises(CvarError):
        ops.lora_wgrad(x, u, out, ws, M=64, N=64, r=16, p=-1.0)                           # p < 0
    with pytest.raises(CvarError):
        ops.lora_dropout_mask(4, 4, 1.0, 0, 0, device=dev)
    # the device is still fine
    ops.lora_down(x, A, u, **down)
    torch.cuda.synchronize()
    assert torch.equal(u, torch.full_like(u, 64.0))
