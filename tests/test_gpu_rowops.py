"""Every launcher of csrc/ops.h, csrc/select.h and csrc/rl.h, and the classifier GEMM's two fused epilogues, one by
one through the capgen_debug_* hooks against a float64 restatement of the formula in the header
comments (never the library itself), at the smallest shapes that reach every template
instantiation and launcher branch.  Inputs come from fixed-seed CPU generators; bf16 cases hand
the reference the bf16-rounded inputs.  Where the expected result is an index (argmax, top-k),
the test first asserts ON THE REFERENCE that the competing scores are >= 1e-4 apart, so float32
rounding cannot change the answer; exact ties are pinned in tests of their own.

Tolerances (f32 unit roundoff 6e-8 through reductions of <= 1024 terms leaves two orders of
headroom; one element of 1024 dropped from a mean moves it by 1e-3):
  f32 outputs   |got - ref| <= 1e-5 max|ref| of the tensor (loss rows: 1e-5 (|lse| + |tlogit|))
  bf16 outputs  + 2^-8 |ref| elementwise (one output rounding)
  exact         integer outputs, bf16 shadow / tiled copy, guard regions, zero rows, checksums
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = 0, 1
TDT = {F32: torch.float32, BF16: torch.bfloat16}
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def _lib_():
    from capgen import _lib
    return _lib, _lib.load()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    _lib, lib = _lib_()
    _lib.check(getattr(lib, name)(*args))
    torch.cuda.synchronize()


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def dev(t):
    return None if t is None else t.to(DEV)


def rnd(t, dtype):
    """the input as the kernel's dtype stores it, and the float64 value of that"""
    s = t.to(TDT[dtype])
    return s, s.double()


def assert_close(got, ref, dtype=F32, what="", extra=None):
    """f32: 1e-5 max|ref|; bf16: plus one output rounding 2^-8 |ref|; extra: a further elementwise bound"""
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    bound = 1e-5 * ref.abs().max().clamp_min(1e-30) + torch.zeros_like(ref)
    if dtype == BF16:
        bound = bound + 2.0 ** -8 * ref.abs()
    if extra is not None:
        bound = bound + extra
    err = (got - ref).abs()
    bad = err > bound
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} (bound there " \
                          f"{bound.flatten()[err.argmax()].item():.3e}), {int(bad.sum())} of {bad.numel()} out"


def assert_same(got, ref, what=""):
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.dtype == torch.bfloat16:  # bit patterns (so -0.0 / NaN patterns count)
        got, ref = got.view(torch.int16), ref.view(torch.int16)
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {got.numel()} elements differ"


# ---- the dropout mask, restated from the comments of capgen_common.h ---------------------------------
def lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def drop_keep(seed, site, n, p):
    """keep[idx] for idx = m * d + col < n"""
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    key = lowbias32(lo ^ int(lowbias32((hi + 0x9E3779B9 * (site + 1)) & 0xFFFFFFFF)))
    thresh = min(int(np.floor(float(np.float32(p)) * 2.0 ** 32)), 0xFFFFFFFF)
    idx = np.arange(n, dtype=np.uint64)
    return lowbias32(idx ^ key) >= np.uint64(thresh)


SEEDS = [0x0123456789ABCDEF, 7, 0xFFFFFFFF00000001]
SITES = [0, 5]
DROP_P = 0.3


@pytest.mark.parametrize("n", [37 * 64, 37 * 1024])
def test_dropout_restatement_keep_share(n):
    """A condition on the restatement, not on the kernel: its keep share is within 4 binomial
    standard deviations of 1 - p (measured on the CPU: within 1.2 in every case)."""
    sd = np.sqrt(0.7 * 0.3 / n)
    for seed in SEEDS:
        for site in SITES:
            share = drop_keep(seed, site, n, DROP_P).mean()
            assert abs(share - 0.7) <= 4 * sd, (hex(seed), site, share)
    # (and the masks of different seeds / sites are different masks)
    a = drop_keep(SEEDS[0], 0, n, DROP_P)
    assert (a != drop_keep(SEEDS[0], 5, n, DROP_P)).mean() > 0.3
    assert (a != drop_keep(SEEDS[1], 0, n, DROP_P)).mean() > 0.3


# ---- LayerNorm ---------------------------------------------------------------------------------------
LN_DS = [64, 128, 256, 512, 1024]  # DPL = 1, 2, 4, 8, 16
LN_MS = [1, 5, 37]                 # 37: no multiple of the 4 (forward) / 8 (backward) rows per workgroup
LN_EPS = 1e-6
PE_L = 5
PAD = 2


def ln_case(M, d, dtype, opts, seed, site):
    """inputs of one LayerNorm case (CPU tensors as the kernel stores them + their float64 values)"""
    g = gen(1000 * d + 10 * M + dtype)
    # rows of different scale: a row of variance 2.5e-3 or 1e-4 makes the epsilon matter
    rs = torch.tensor([1.0, 0.05, 0.01])[torch.arange(M) % 3].unsqueeze(1)
    c = {"M": M, "d": d, "dtype": dtype}
    c["a"], c["a64"] = rnd(torch.randn(M, d, generator=g) * rs + 0.1, dtype)
    c["gamma"] = 1 + 0.3 * torch.randn(d, generator=g)
    c["beta"] = 0.2 * torch.randn(d, generator=g)
    full = opts == "all"
    c["bias"] = 0.5 * torch.randn(d, generator=g) if full else None
    c["res"], c["res64"] = rnd(torch.randn(M, d, generator=g), dtype) if full else (None, None)
    c["pe"] = None
    if full:  # pe_L rows and one more that a wrong row index (m % pe_L is the rule) would read
        c["pe"] = torch.cat([torch.randn(PE_L, d, generator=g), torch.full((1, d), 1e3)])
    c["ids"] = None
    c["valid"] = None
    keep_row = torch.ones(M, dtype=torch.bool)
    if full:
        ids = torch.randint(3, 50, (M, 3), generator=g, dtype=torch.int32)
        ids[:, 1:] = PAD  # only column 0 (ids_ld = 3) is the row's id
        for m in {0, M - 1, M // 2, 7 % M}:
            ids[m, 0] = PAD
            ids[m, 1:] = 9
        c["ids"] = ids
        keep_row = ids[:, 0] != PAD
    if opts == "valid":
        v = torch.ones(M, dtype=torch.uint8)
        v[[m for m in {0, M - 1, 3 % M}]] = 0
        if M > 1:
            v[1] = 1
        c["valid"] = v
        keep_row = v != 0
    c["keep_row"] = keep_row
    c["drop"] = None
    if full:
        c["drop"] = (DROP_P, site, seed)
        c["keep"] = torch.from_numpy(drop_keep(seed, site, M * d, DROP_P).reshape(M, d))
        c["scale"] = float(np.float32(1.0) / (np.float32(1.0) - np.float32(DROP_P)))
    return c


def ln_input64(c, a, bias, res):
    """the LayerNorm input v = drop(a + a_bias) + res + pe[m % pe_L] in float64 (ops.h LnFwd)"""
    x = a
    if bias is not None:
        x = x + bias
    if c["drop"] is not None:
        x = torch.where(c["keep"], x * c["scale"], torch.zeros_like(x))
    if res is not None:
        x = x + res
    if c["pe"] is not None:
        x = x + c["pe"][:PE_L].double()[torch.arange(c["M"]) % PE_L]
    return x


def ln_norm64(c, x, gamma, beta):
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    y = ((x - mean) * rstd * gamma + beta) * c["keep_row"].double().unsqueeze(1)
    return y, mean.squeeze(1), rstd.squeeze(1)


def drop_args(c):
    p, site, seed = c["drop"] if c["drop"] is not None else (0.0, 0, 0)
    return C.c_float(p), site, C.c_uint64(seed)


def ln_combos(opts, M):
    if opts != "all":
        return [(0, 0)]
    if M != 37:
        return [(SEEDS[M % 3], SITES[M % 2])]
    return [(s, t) for s in SEEDS for t in SITES]


@gpu
@pytest.mark.parametrize("opts", ["bare", "all", "valid"])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("d", LN_DS)
def test_layernorm_fwd(d, dtype, opts):
    for M in LN_MS:
        for seed, site in ln_combos(opts, M):
            c = ln_case(M, d, dtype, opts, seed, site)
            x = ln_input64(c, c["a64"], None if c["bias"] is None else c["bias"].double(), c["res64"])
            y, mean, rstd = ln_norm64(c, x, c["gamma"].double(), c["beta"].double())
            tag = f"M={M} d={d} dtype={dtype} {opts} seed={seed:#x} site={site}"
            td = TDT[dtype]
            yd = torch.full((M + 1, d), 7.0, dtype=td, device=DEV)  # (a guard row behind each output)
            vd = torch.full((M + 1, d), 7.0, dtype=td, device=DEV)
            md = torch.full((M + 1,), 7.0, device=DEV)
            rd = torch.full((M + 1,), 7.0, device=DEV)
            ins = {k: dev(c[k]) for k in ("a", "bias", "res", "pe", "gamma", "beta", "ids", "valid")}
            call("capgen_debug_layernorm_fwd", dtype, M, d, P(ins["a"]), P(ins["bias"]), *drop_args(c), P(ins["res"]),
                 P(ins["pe"]), PE_L, P(ins["gamma"]), P(ins["beta"]), P(ins["ids"]), 3, PAD, P(ins["valid"]), P(yd),
                 P(vd), P(md), P(rd), None)
            assert_close(yd[:M], y, dtype, tag + " y")
            assert_close(vd[:M], x, dtype, tag + " v_save")
            assert_close(md[:M], mean, F32, tag + " mean")
            assert_close(rd[:M], rstd, F32, tag + " rstd")
            masked = ~c["keep_row"]
            if opts != "bare":
                assert masked.any() and (M == 1 or not masked.all())
            assert (yd[:M].cpu()[masked] == 0).all(), tag + ": a masked row is exactly zero"
            for o in (yd, vd, md, rd):
                assert (o[M:] == 7.0).all(), tag + ": guard row written"


def stripe_buf(g, stripes, stride, d):
    """striped accumulators: random non-zero prefill in the d used columns, 99 in the guard columns"""
    b = torch.full((stripes, stride), 99.0)
    b[:, :d] = torch.randn(stripes, d, generator=g) + 3
    return b


@gpu
@pytest.mark.parametrize("opts", ["bare", "all", "valid", "d_res_only", "d_a_only", "no_sums"])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("d", LN_DS)
def test_layernorm_bwd(d, dtype, opts):
    """Reference: torch float64 autograd through the forward restatement above (not the backward
    formula of the kernel).  The kernel takes v, mean and rstd from the test: v as the dtype stores
    it, mean / rstd the statistics of exactly that v."""
    fopts = opts if opts in ("bare", "all", "valid") else "all"
    td = TDT[dtype]
    for M in LN_MS:
        for stripes in (1, 3):
            seed, site = ln_combos(fopts, M)[(stripes + d // 64) % len(ln_combos(fopts, M))]
            c = ln_case(M, d, dtype, fopts, seed, site)
            g = gen(77 * d + M + stripes)
            tag = f"M={M} d={d} dtype={dtype} {opts} stripes={stripes} seed={seed:#x} site={site}"
            a = c["a64"].clone().requires_grad_(True)
            bias = None if c["bias"] is None else c["bias"].double().requires_grad_(True)
            res = None if c["res64"] is None else c["res64"].clone().requires_grad_(True)
            gamma = c["gamma"].double().requires_grad_(True)
            beta = c["beta"].double().requires_grad_(True)
            x = ln_input64(c, a, bias, res)
            v_st, v64 = rnd(x.detach().float(), dtype)
            xin = x + (v64 - x).detach()  # the value the kernel is given, the graph of the forward
            xin.retain_grad()
            y, mean, rstd = ln_norm64(c, xin, gamma, beta)
            dy_st, dy64 = rnd(torch.randn(M, d, generator=g), dtype)
            (y * dy64).sum().backward()
            want_res = opts != "d_a_only"
            want_a = opts != "d_res_only"
            want_sums = opts != "no_sums"
            want_dbias = want_sums and want_a
            stride = d + 24
            acc = {k: stripe_buf(g, stripes, stride, d) for k in ("dgamma", "dbeta", "dbias")}
            accd = {k: dev(v) for k, v in acc.items()}
            dres = torch.full((M + 1, d), 7.0, dtype=td, device=DEV) if want_res else None
            da = torch.full((M + 1, d), 7.0, dtype=td, device=DEV) if want_a else None
            ins = {k: dev(c[k]) for k in ("gamma", "ids", "valid")}
            dyd, vd = dev(dy_st), dev(v_st)
            md, rd = dev(mean.detach().float()), dev(rstd.detach().float())
            call("capgen_debug_layernorm_bwd", dtype, M, d, P(dyd), P(vd), P(md), P(rd), P(ins["gamma"]),
                 P(ins["ids"]), 3, PAD, P(ins["valid"]), *drop_args(c), P(dres), P(da),
                 P(accd["dgamma"]) if want_sums else None, P(accd["dbeta"]) if want_sums else None,
                 P(accd["dbias"]) if want_dbias else None, stripes, stride, None)
            if want_res:
                assert_close(dres[:M], xin.grad, dtype, tag + " d_res")
                assert (dres[M:] == 7.0).all(), tag
            if want_a:
                assert_close(da[:M], a.grad, dtype, tag + " d_a")
                assert (da[M:] == 7.0).all(), tag
                if c["drop"] is not None:  # the backward drops exactly the elements the forward dropped
                    assert (da[:M].cpu()[~c["keep"]] == 0).all(), tag + ": dropped elements carry no gradient"
            ref_sums = {"dgamma": gamma.grad, "dbeta": beta.grad, "dbias": a.grad.sum(0)}
            for k in ("dgamma", "dbeta", "dbias"):
                got = accd[k].cpu()
                assert (got[:, d:] == 99.0).all(), tag + f" {k}: guard between the stripes written"
                if not want_sums or (k == "dbias" and not want_dbias):
                    assert torch.equal(got, acc[k]), tag + f" {k}: must not be touched"
                    continue
                # the accumulators accumulate: fold the stripes (stripe_reduce) and take the prefill off
                dst = torch.full((d + 1,), 5.0, device=DEV)
                call("capgen_debug_stripe_reduce", P(accd[k]), stripes, stride, d, P(dst), 0, 0, None)
                assert dst[d].item() == 5.0
                assert_close(dst[:d], acc[k][:, :d].double().sum(0) + ref_sums[k], F32, tag + " " + k)


# ---- stripe_reduce / column_sum ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 300_000])  # 300 000: past one pass of the 1024-workgroup grid
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("clear", [0, 1])
def test_stripe_reduce(n, accumulate, clear):
    g = gen(n + accumulate * 2 + clear)
    stripes, stride = 3, n + 8
    S = torch.full((stripes, stride), 99.0)
    S[:, :n] = torch.randn(stripes, n, generator=g)
    dst0 = torch.randn(n + 1, generator=g)
    Sd, dd = dev(S), dev(dst0)
    call("capgen_debug_stripe_reduce", P(Sd), stripes, stride, n, P(dd), accumulate, clear, None)
    ref = S[:, :n].double().sum(0) + (dst0[:n].double() if accumulate else 0)
    assert_close(dd[:n], ref, F32, "dst")
    assert dd[n].item() == dst0[n].item(), "element past n written"
    got = Sd.cpu()
    assert (got[:, n:] == 99.0).all(), "guard between the stripes written"
    if clear:
        assert (got[:, :n] == 0).all(), "partials not zeroed"
    else:
        assert torch.equal(got, S), "partials changed without clear"


@gpu
@pytest.mark.parametrize("stripes", [1, 3])
@pytest.mark.parametrize("with_ptr", [0, 1])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("M,N", [(1, 8), (255, 40), (257, 72), (600, 520)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_column_sum(dtype, M, N, wide, with_ptr, stripes):
    g = gen(M * 13 + N + dtype)
    ldx = N + 16 * wide
    X = torch.randn(M, ldx, generator=g)
    X[:, N:] = 1e6  # (columns past N are not part of the sum)
    X_st, X64 = rnd(X, dtype)
    alpha, ap = 0.75, torch.tensor([-1.7])
    stride = N + 8
    db0 = torch.full((stripes, stride), 99.0)
    db0[:, :N] = torch.randn(stripes, N, generator=g)
    Xd, dbd, apd = dev(X_st), dev(db0), dev(ap)
    call("capgen_debug_column_sum", dtype, P(Xd), M, N, ldx, C.c_float(alpha), P(apd) if with_ptr else None, P(dbd),
         stripes, stride, None)
    a = alpha * (float(ap[0]) if with_ptr else 1.0)
    got = dbd.cpu()
    assert (got[:, N:] == 99.0).all(), "guard between the stripes written"
    ref = db0[:, :N].double().sum(0) + a * X64[:, :N].sum(0)
    # each stripe holds whole 256-row blocks (block b in stripe b % stripes); their sum is the column sum
    assert_close(got[:, :N].double().sum(0), ref, F32, "column sums")
    if stripes == 3 and M > 512:
        for s in range(3):
            part = db0[s, :N].double() + a * X64[256 * s:256 * (s + 1), :N].sum(0)
            assert_close(got[s, :N], part, F32, f"stripe {s}")


# ---- embedding ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", [64, 520])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ids_ld", [1, 3])
def test_embedding_gather(ids_ld, dtype, d):
    g = gen(d + ids_ld)
    R, M = 40, 37
    table = torch.randn(R, d, generator=g)
    ids = torch.randint(0, R, (M, ids_ld), generator=g, dtype=torch.int32)
    ids[0, 0], ids[1, 0] = 0, R - 1
    if ids_ld > 1:
        ids[:, 1:] = (ids[:, :1] + 1) % R  # a kernel ignoring the stride reads these
    out = torch.full((M + 1, d), 7.0, dtype=TDT[dtype], device=DEV)
    td, idd = dev(table), dev(ids)
    call("capgen_debug_embedding_gather", P(td), P(idd), ids_ld, M, d, P(out), dtype, None)
    assert_same(out[:M], table[ids[:, 0].long()].to(TDT[dtype]), "gathered rows")
    assert (out[M:] == 7.0).all()
    assert torch.equal(td.cpu(), table)


@gpu
@pytest.mark.parametrize("d", [64, 520])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_embedding_scatter_add(dtype, d):
    g = gen(d + dtype)
    R, M, pad = 12, 50, 4
    ids = torch.randint(2, R - 2, (M,), generator=g, dtype=torch.int32)  # rows 0, 1, R-2, R-1: guards
    ids[:6] = torch.tensor([5, 5, 5, pad, pad, 2], dtype=torch.int32)
    dE_st, dE64 = rnd(torch.randn(M, d, generator=g), dtype)
    grad0 = torch.randn(R, d, generator=g)
    gd, dEd, idd = dev(grad0), dev(dE_st), dev(ids)
    call("capgen_debug_embedding_scatter_add", P(dEd), P(idd), M, d, pad, P(gd), dtype, None)
    ref = grad0.double()
    for m in range(M):
        if ids[m] != pad:
            ref[ids[m]] += dE64[m]
    got = gd.cpu()
    assert_close(got, ref, F32, "embedding gradient")
    for r in (0, 1, pad, R - 2, R - 1):
        assert torch.equal(got[r], grad0[r]), f"row {r} (guard / pad id) changed"


# ---- pack_encoder_input / prepare_captions -----------------------------------------------------------
@gpu
@pytest.mark.parametrize("indexed", [0, 1])
@pytest.mark.parametrize("P_", [4, 5])
@pytest.mark.parametrize("F", [8, 520, 2048])
@pytest.mark.parametrize("ft,ot", [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)])
def test_pack_encoder_input(ft, ot, F, P_, indexed):
    g = gen(F + P_ + 2 * ft + ot)
    Kp = (F + P_ + 31) // 32 * 32
    N, n_img = 3, 3
    rows = n_img * N  # the store: 9 rows (no multiple of the 4 rows per workgroup)
    feats, feats64 = rnd(torch.randn(rows, F, generator=g), ft)
    pos = torch.randn(rows, P_, generator=g)
    pos[1] = 0.0
    pos[4] = 0.0
    pos[4, P_ - 1] = -0.0  # a row holding only zeros, one of them negative: padding (pos != 0 is false)
    pos[7] = 0.0
    pos[7, 0] = 1e-30      # not padding
    if indexed:
        img_idx = torch.tensor([1, -1, n_img, 0, 2], dtype=torch.int32)
        M = len(img_idx) * N
        src = [(int(i) * N + n if 0 <= int(i) < n_img else -1) for i in img_idx for n in range(N)]
    else:
        img_idx, M = None, rows
        src = list(range(rows))
    ref = torch.zeros(M, Kp, dtype=torch.float64)
    valid = torch.zeros(M, dtype=torch.uint8)
    for m, s_ in enumerate(src):
        if s_ < 0:
            continue
        ref[m, :F] = feats64[s_]
        ref[m, F:F + P_] = pos[s_].double()
        valid[m] = 1 if (pos[s_] != 0).any() else 0
    out = torch.full((M + 1, Kp), 7.0, dtype=TDT[ot], device=DEV)
    vd = torch.full((M + 1,), 9, dtype=torch.uint8, device=DEV)
    seed0 = 0xFEDCBA9876543210
    sb = torch.from_numpy(np.array([seed0], dtype=np.uint64).view(np.int64)).to(DEV)
    fd, pd, idd = dev(feats), dev(pos), dev(img_idx)
    call("capgen_debug_pack_encoder_input", P(fd), ft, P(pd), M, F, P_, Kp, P(out), ot, P(vd), P(idd), N if indexed else 0,
         n_img if indexed else 0, P(sb), None)
    assert_same(out[:M], ref.to(TDT[ot]), "packed rows")  # (a conversion of exact values: no tolerance)
    assert_same(vd[:M], valid, "valid")
    assert 0 < int(valid.sum()) < M
    assert (out[M:] == 7.0).all() and vd[M].item() == 9
    assert int(sb.cpu().numpy().view(np.uint64)[0]) == (seed0 + GOLD) & M64, "seed_bump advances exactly once"
    if indexed:
        dead = [m for m, s_ in enumerate(src) if s_ < 0]
        assert len(dead) == 2 * N and (out[dead].float() == 0).all() and (vd[dead] == 0).all()


@gpu
@pytest.mark.parametrize("B,T", [(1, 2), (3, 10), (70, 21)])  # 70 x 20 > the 1024 threads of the launch
def test_prepare_captions(B, T):
    g = gen(B * 31 + T)
    pad = 0
    caps = torch.randint(1, 50, (B, T), generator=g, dtype=torch.int32)
    for b in range(B):  # trailing padding of different lengths, never a whole caption
        n = int(torch.randint(0, T - 1, (1,), generator=g))
        if n:
            caps[b, T - n:] = pad
    L = T - 1
    ids = torch.full((B * L + 1,), -7, dtype=torch.int32, device=DEV)
    tgt = torch.full((B * L + 1,), -7, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(2, device=DEV)
    inv = torch.zeros(2, device=DEV)
    seed0 = 12345
    sb = torch.tensor([seed0], dtype=torch.int64, device=DEV)
    cd = dev(caps)
    call("capgen_debug_prepare_captions", P(cd), B, T, pad, P(ids), P(tgt), P(cnt), P(sb), P(inv), None)
    assert_same(ids[:B * L], caps[:, :-1].reshape(-1).contiguous(), "ids_in")
    assert_same(tgt[:B * L], caps[:, 1:].reshape(-1).contiguous(), "targets")
    assert ids[B * L].item() == -7 and tgt[B * L].item() == -7
    n = int((caps[:, 1:] != pad).sum())
    assert n > 0
    assert cnt[0].item() == float(n) and cnt[1].item() == 0
    assert abs(inv[0].item() - 1.0 / n) <= 1e-5 / n and inv[1].item() == 0
    assert int(sb.cpu().numpy().view(np.uint64)[0]) == (seed0 + GOLD) & M64
    # inv_count is optional
    call("capgen_debug_prepare_captions", P(cd), B, T, pad, P(ids), P(tgt), P(cnt), None, None, None)
    assert cnt[0].item() == float(n)


# ---- cross entropy -----------------------------------------------------------------------------------
CE_PAD = 1


def ce_rows(V, seed):
    """M = 6 logit rows and targets: columns 0, V-1, both sides of a float4 boundary, a pad row, and a
    row of values near -60 with one +60 (the row maximum must be subtracted)"""
    g = gen(seed)
    x = 2 * torch.randn(6, V, generator=g)
    x[4] = -60 + torch.randn(V, generator=g)
    x[4, V // 2] = 60.0
    tgt = torch.tensor([0, V - 1, 4, CE_PAD, 3, V // 2], dtype=torch.int32)
    return x, tgt


def ce_ref(x64, tgt, pad):
    lse = torch.logsumexp(x64, 1)
    tl = x64[torch.arange(len(tgt)), tgt.long()]
    kept = (tgt != pad).double()
    sm = torch.exp(x64 - lse.unsqueeze(1))
    grad = sm.clone()
    grad[torch.arange(len(tgt)), tgt.long()] -= 1
    return lse, tl, (lse - tl) * kept, grad * kept.unsqueeze(1), sm


def assert_loss_rows(got, lse, tl, tgt, pad, what):
    got = got.cpu().double()
    kept = tgt != pad
    bound = 1e-5 * (lse.abs() + tl.abs())
    assert ((got - (lse - tl)).abs() <= bound)[kept].all(), (what, got, lse - tl)
    assert (got[~kept] == 0).all(), what + ": the loss of a pad row is 0"


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("V", [8, 1000, 4100, 8200, 10000, 16384, 10, 1001, 16388])
def test_cross_entropy_rows(V, dtype):
    """V % 4 == 0: the register-resident form with NV4 = 4 (8, 1000), 8 (4100, 8200), 10 (10000) and
    16 (16384); otherwise (and past 16384) the generic three-pass form."""
    x, tgt = ce_rows(V, V)
    lse, tl, loss, grad, _ = ce_ref(x.double(), tgt, CE_PAD)
    M = 6
    lr = torch.full((M + 1,), 7.0, device=DEV)
    dl = torch.full((M * V + 8,), 7.0, dtype=TDT[dtype], device=DEV)
    xd, td = dev(x), dev(tgt)
    call("capgen_debug_cross_entropy_rows", P(xd), P(td), M, V, CE_PAD, P(lr), P(dl), dtype, None)
    assert_loss_rows(lr[:M], lse, tl, tgt, CE_PAD, f"V={V}")
    assert lr[M].item() == 7.0 and (dl[M * V:] == 7.0).all()
    got = dl[:M * V].view(M, V)
    assert_close(got, grad, dtype, f"V={V} softmax - onehot")
    assert (got[3].cpu() == 0).all(), "the gradient of a pad row is exactly zero"


def slab_stats(x):
    """what the classifier epilogues leave per row and 16-column slab (gemm.h GemmArgs::ce_stats):
    mx = max(v), s = sum exp(v - mx) (f32), e = bf16(exp(v - mx))"""
    M, V = x.shape
    S = (V + 15) // 16
    xp = torch.full((M, S * 16), -float("inf"), dtype=torch.float64)
    xp[:, :V] = x.double()
    xs = xp.view(M, S, 16)
    mx = xs.max(2).values
    ex = torch.exp(xs - mx.unsqueeze(2))
    stats = torch.stack([mx, ex.sum(2)], 2).float()  # [M][S]{mx, s}
    e = ex.view(M, S * 16)[:, :V].float().bfloat16()
    return stats, e


def run_ce_finish(stats, e, tl, tgt, V, pad, ld):
    M, S = stats.shape[:2]
    st = torch.full((M, ld, 2), float("nan"))
    st[:, :S] = stats
    dl = torch.full((M * V + 16,), 7.0, dtype=torch.bfloat16)
    dl[:M * V] = e.reshape(-1)
    lr = torch.full((M + 1,), 7.0, device=DEV)
    std, dld, tld, td = dev(st), dev(dl), dev(tl.float()), dev(tgt)
    call("capgen_debug_ce_finish", P(std), ld, P(tld), P(td), M, V, pad, P(lr), P(dld), None)
    assert lr[M].item() == 7.0
    # the columns of a partial last slab beyond V do not exist: the element after the last row stays
    assert (dld[M * V:] == 7.0).all(), "ce_finish wrote past the last row"
    return lr[:M], dld[:M * V].view(M, V)


CE_FINISH_VS = [8, 24, 1000, 4104, 8200, 12296, 16392, 12, 1004]


@gpu
@pytest.mark.parametrize("wide_ld", [0, 1])
@pytest.mark.parametrize("V,vec8", [(V, 1) for V in CE_FINISH_VS] + [(V, 0) for V in CE_FINISH_VS if V % 8 == 0])
def test_ce_finish(V, vec8, wide_ld, set_knob):
    """SPT = 1 (8 .. 1000), 2 (4104), 3 (8200), 4 (12296), 8 (16392); V = 12, 1004 (V % 8 != 0) take the
    8-byte form, which CE_VEC8 = 0 forces for every V.  The result entries are rounded twice (e, then
    the output): 2^-7 softmax, and the target entry is near -1: 2^-8 more there."""
    set_knob("CE_VEC8", vec8)
    x, tgt = ce_rows(V, V + 1)
    stats, e = slab_stats(x)
    lse, tl, loss, grad, sm = ce_ref(x.double(), tgt, CE_PAD)
    S = stats.shape[1]
    lr, got = run_ce_finish(stats, e, tl, tgt, V, CE_PAD, S + 3 * wide_ld)
    assert_loss_rows(lr, lse, tl, tgt, CE_PAD, f"V={V}")
    onehot = torch.zeros_like(sm)
    onehot[torch.arange(6), tgt.long()] = 1
    assert_close(got, grad, F32, f"V={V} softmax - onehot", extra=2.0 ** -7 * sm + 2.0 ** -8 * onehot)
    assert (got[3].cpu().float() == 0).all(), "the gradient of a pad row is exactly zero"


@gpu
def test_ce_finish_rejects_bad_shapes():
    _lib, lib = _lib_()
    z = torch.zeros(64, device=DEV)
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.capgen_debug_ce_finish(P(z), 1, P(z), P(zi), 1, 10, 0, P(z), P(z), None) == 1  # V % 4 != 0
    assert b"ce_finish" in lib.capgen_last_error()
    assert lib.capgen_debug_ce_finish(P(z), 1, P(z), P(zi), 1, 32, 0, P(z), P(z), None) == 1  # ld < slabs


# ---- the classifier GEMM's fused epilogues ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("V", [24, 1000])  # 1000: a last slab of 8 columns
@pytest.mark.parametrize("M", [5, 130])
def test_classifier_epilogues(M, V):
    """bf16 NT GEMM + f32 bias with GemmArgs::ce_stats (training) and ::dec_stats (decode), then the
    ce_stats outputs through ce_finish.  Bound on the logits: the project's bf16 GEMM bound
    2e-3 sqrt(K); slab maxima, tlogit and the log-sum-exp are 1-Lipschitz in the logits."""
    K, pad = 64, 0
    g = gen(M + V)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = (0.3 * torch.randn(V, K, generator=g)).bfloat16()
    bias = torch.randn(V, generator=g)
    tgt = torch.randint(1, V, (M,), generator=g, dtype=torch.int32)
    tgt[0], tgt[M - 1], tgt[1] = V - 1, 0 + 1, pad
    tgt[2] = 15
    v = A.double() @ W.double().t() + bias.double()
    b = 2e-3 * np.sqrt(K)
    S = (V + 15) // 16
    ref_stats, _ = slab_stats(v)
    ref_lse = torch.logsumexp(v, 1)
    Ad, Wd, bd, td = dev(A), dev(W), dev(bias), dev(tgt)

    def check_stats(st, what):
        st = st.cpu().double()
        assert ((st[:, :, 0] - ref_stats[:, :, 0].double()).abs() <= b).all(), what + " slab max"
        lse = torch.logsumexp(st[:, :, 0] + torch.log(st[:, :, 1]), 1)
        assert ((lse - ref_lse).abs() <= b).all(), what + " log sum_c s_c exp(mx_c)"

    # training form: C = bf16 exp(v - slab max)
    e = torch.full((M * V + 16,), 7.0, dtype=torch.bfloat16, device=DEV)
    st = torch.full((M + 1, S, 2), 7.0, device=DEV)
    tl = torch.full((M + 1,), 7.0, device=DEV)
    call("capgen_debug_gemm_classifier", M, V, K, P(Ad), K, P(Wd), K, P(e), V, P(bd), P(st), S, P(td), P(tl), None)
    assert (e[M * V:] == 7.0).all() and (st[M:] == 7.0).all() and tl[M].item() == 7.0
    check_stats(st[:M], "ce_stats")
    ref_tl = v[torch.arange(M), tgt.long()]
    assert ((tl[:M].cpu().double() - ref_tl).abs() <= b).all(), "tlogit"
    ev = e[:M * V].view(M, V).cpu().double()
    mxc = st[:M, :, 0].cpu().double().repeat_interleave(16, 1)[:, :V]
    rel = np.exp(b) - 1 + 2.0 ** -8
    assert ((ev * torch.exp(mxc) - torch.exp(v)).abs() <= rel * torch.exp(v)).all(), "e * exp(mx) against exp(v)"
    # decode form: C = the f32 logits
    lg = torch.full((M * V + 16,), 7.0, device=DEV)
    st2 = torch.full((M + 1, S, 2), 7.0, device=DEV)
    call("capgen_debug_gemm_classifier", M, V, K, P(Ad), K, P(Wd), K, P(lg), V, P(bd), P(st2), S, None, None, None)
    assert (lg[M * V:] == 7.0).all() and (st2[M:] == 7.0).all()
    check_stats(st2[:M], "dec_stats")
    lgc = lg[:M * V].view(M, V).cpu()
    assert ((lgc.double() - v).abs() <= b).all(), "decode logits"
    own, _ = slab_stats(lgc)  # and the stats are those of the logits it stored
    assert_close(st2[:M, :, 0], own[:, :, 0].double(), F32, "dec_stats max of the stored logits")
    assert ((st2[:M, :, 1].cpu().double() - own[:, :, 1].double()).abs() <= 1e-5 * own[:, :, 1].double()).all()
    # chained: ce_stats -> ce_finish against the float64 cross entropy.  lse and tlogit are each within
    # b, so the loss row is within 2 b and softmax within exp(2 b) - 1 relative, plus ce_finish's own
    # roundings (2^-7 softmax, 2^-8 at the target)
    lr = torch.full((M,), 7.0, device=DEV)
    call("capgen_debug_ce_finish", P(st), S, P(tl), P(td), M, V, pad, P(lr), P(e), None)
    lse, _, loss, grad, sm = ce_ref(v, tgt, pad)
    assert ((lr.cpu().double() - loss).abs() <= 2 * b).all(), "chained loss rows"
    onehot = torch.zeros_like(sm)
    onehot[torch.arange(M), tgt.long()] = 1
    kept = (tgt != pad).double().unsqueeze(1)
    got = e[:M * V].view(M, V)
    assert_close(got, grad, F32, "chained softmax - onehot",
                 extra=((np.exp(2 * b) - 1 + 2.0 ** -7) * sm + 2.0 ** -8 * onehot) * kept)
    assert (got[1].cpu().float() == 0).all() and lr[1].item() == 0


# ---- loss_finalize -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M", [1, 300])
def test_loss_finalize(M):
    g = gen(M)
    rows = 3 * torch.rand(M, generator=g) + 0.5
    n = float(max(1, M - 3))
    rd, cd = dev(rows), torch.tensor([n], device=DEV)
    ce = rows.double().sum().item() / n

    def run(focal, ce_in=None, partial=0, want_scale=True):
        out = torch.full((2,), 7.0, device=DEV)
        gs = torch.full((2,), 7.0, device=DEV)
        cin = None if ce_in is None else torch.tensor([ce_in], device=DEV)
        call("capgen_debug_loss_finalize", P(rd), M, P(cd), focal, P(out), P(gs) if want_scale else None, P(cin),
             partial, None)
        assert out[1].item() == 7.0 and gs[1].item() == 7.0
        return out[0].item(), gs[0].item()

    def focal_ref(c):
        c = torch.tensor(c, dtype=torch.float64, requires_grad=True)
        loss = (1 - torch.exp(-c)) ** 2 * c
        loss.backward()
        return loss.item(), c.grad.item() / n  # d loss / d(sum of rows) = loss'(ce) / count

    def near(a, b):
        return abs(a - b) <= 1e-5 * abs(b)

    loss, gs = run(0)
    assert near(loss, ce) and near(gs, 1 / n)
    loss, gs = run(1)
    fl, fg = focal_ref(ce)
    assert near(loss, fl) and near(gs, fg), (loss, fl, gs, fg)
    given = float(np.float32(1.37))  # ce_in: the rows are not read
    loss, gs = run(0, ce_in=given)
    assert near(loss, given) and near(gs, 1 / n)
    loss, gs = run(1, ce_in=given)
    fl, fg = focal_ref(given)
    assert near(loss, fl) and near(gs, fg)
    loss, gs = run(1, partial=1)  # partial: the mean only, whatever focal says; no scale
    assert near(loss, ce) and gs == 7.0
    loss, gs = run(1, want_scale=False)
    assert near(loss, focal_ref(ce)[0]) and gs == 7.0


# ---- Adam --------------------------------------------------------------------------------------------
LR, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))


def adam_ref(p, grads):
    """torch's single-tensor Adam (no weight decay, no amsgrad) in float64, from zero moments"""
    p = p.clone()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    out = []
    for t, g in enumerate(grads, 1):
        m = m + (g - m) * (1 - B1)                       # exp_avg.lerp_(grad, 1 - beta1)
        v = v * B2 + (1 - B2) * g * g                    # exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
        denom = v.sqrt() / np.sqrt(1 - B2 ** t) + EPS    # (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        p = p - (LR / (1 - B1 ** t)) * m / denom         # param.addcdiv_(exp_avg, denom, value=-step_size)
        out.append((p.clone(), m.clone(), v.clone()))
    return out


def adam_inputs(n, seed):
    g = gen(seed)
    p = torch.randn(n, generator=g)
    grads = []
    for t in range(3):
        gr = torch.randn(n, generator=g) * (0.1 + t)
        gr[0::7] = 0.0                                   # exactly zero
        gr[1::7] = 1e-12 * (1 - 2 * (t % 2))             # eps-dominated, changing sign
        grads.append(gr)
    return p, grads


def test_adam_restatement_matches_torch():
    """anchors the reference of test_adam: the float64 restatement against torch.optim.Adam (CPU)"""
    p, grads = adam_inputs(64, 5)
    q = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=LR, betas=(B1, B2), eps=EPS)
    ref = adam_ref(p.double(), [g.double() for g in grads])
    for t in range(3):
        q.grad = grads[t].double().clone()
        opt.step()
        assert (q.detach() - ref[t][0]).abs().max().item() <= 1e-14
        st = opt.state[q]
        assert (st["exp_avg"] - ref[t][1]).abs().max().item() <= 1e-16
        assert (st["exp_avg_sq"] - ref[t][2]).abs().max().item() <= 1e-16


def tiled_index(rows, K=512):
    """where element (n, k) of a [rows][K] bf16 matrix lives in its MFMA fragment pieces (gemm.h
    gemm_tile_b): piece (j, ks) = 512 elements, lane l holds B[n = 16 j + (l & 15)][k = 32 ks + 8 (l >> 4) + e]"""
    idx = np.empty(rows * K, dtype=np.int64)
    for n in range(rows):
        for k in range(K):
            j, ks = n // 16, k // 32
            lane = (n % 16) + 16 * ((k % 32) // 8)
            idx[n * K + k] = ((j * (K // 32) + ks) * 64 + lane) * 8 + k % 8
    return idx


@gpu
@pytest.mark.parametrize("shadow_frac", [0, 1, 2])
@pytest.mark.parametrize("n", [4, 4100, 1_048_580])
def test_adam(n, shadow_frac):
    """n % 4 == 0 and no multiple of the 4096 elements a workgroup covers per pass; the largest takes
    128 grid-stride passes under grid_cap = 2.  Three steps from zero moments."""
    p0, grads = adam_inputs(n, n)
    ref = adam_ref(p0.double(), [g.double() for g in grads])
    n_shadow = [0, (n // 2 + 3) // 4 * 4, n][shadow_frac]
    big = n > 100_000
    tiles = []
    if big and n_shadow:  # two tiled ranges: 16 and 32 rows of 512, the second at a non-zero 4-aligned offset
        tiles = [(0, 16 * 512), (16 * 512 + 12, 32 * 512)]
    pd, md, vd = dev(p0), torch.zeros(n + 4, device=DEV), torch.zeros(n + 4, device=DEV)
    pd = torch.cat([pd, torch.full((4,), 7.0, device=DEV)])
    sh = torch.full((n + 4,), 7.0, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(2, dtype=torch.int64, device=DEV)
    scal = torch.zeros(3, device=DEV)
    dsts = [torch.full((ln + 8,), 7.0, dtype=torch.bfloat16, device=DEV) for _, ln in tiles]
    nt = len(tiles)
    offs = (C.c_int64 * 4)(*[o for o, _ in tiles])
    lens = (C.c_int64 * 4)(*[ln for _, ln in tiles])
    ptrs = (C.c_void_p * 4)(*[d_.data_ptr() for d_ in dsts])
    for t in range(3):
        gd = dev(grads[t])
        call("capgen_debug_adam", P(pd), P(gd), P(md), P(vd), n, C.c_float(LR), C.c_float(B1), C.c_float(B2),
             C.c_float(EPS), P(step), P(scal), P(sh), n_shadow, 2 if big else 0, nt, offs, lens, ptrs, None)
        rp, rm, rv = ref[t]
        assert step[0].item() == t + 1 and step[1].item() == 0
        got = pd[:n].cpu().double()
        bound = 1e-6 * rp.abs().max().item() + 1e-6 * LR
        assert (got - rp).abs().max().item() <= bound, (t, (got - rp).abs().max().item(), bound)
        assert_close(md[:n], rm, F32, f"step {t + 1} exp_avg")
        assert_close(vd[:n], rv, F32, f"step {t + 1} exp_avg_sq")
        assert (pd[n:] == 7.0).all() and (md[n:] == 0).all() and (vd[n:] == 0).all()
        assert scal[2].item() == 0
        # the bf16 shadow: bf16(p) of the parameters the kernel wrote, exactly, and nothing past n_shadow
        shc = sh.cpu()
        assert_same(shc[:n_shadow], pd[:n_shadow].cpu().bfloat16(), "shadow")
        assert (shc[n_shadow:] == 7.0).all(), "shadow written past n_shadow"
        for (off, ln), d_ in zip(tiles, dsts):
            dc = d_.cpu()
            exp = torch.full((ln,), 7.0, dtype=torch.bfloat16)
            exp[torch.from_numpy(tiled_index(ln // 512))] = shc[off:off + ln]
            assert_same(dc[:ln], exp, f"tiled copy of [{off}, {off + ln})")
            assert (dc[ln:] == 7.0).all(), "tiled copy wrote past its range"
    # eps-dominated and zero-gradient elements moved as the reference says (covered by the bound above
    # only if they are compared at their own scale: the update is ~1e-7 there)
    sel = torch.arange(1, n, 7)
    if len(sel):
        d_got = (pd[:n].cpu().double() - p0.double())[sel]
        d_ref = (ref[2][0] - p0.double())[sel]
        assert ((d_got - d_ref).abs() <= 1e-6 * p0.double().abs()[sel] + 1e-6 * LR).all()
    assert torch.equal(pd[:n].cpu()[0::7], p0[0::7]), "a parameter whose gradient was always 0 moved"


@gpu
def test_adam_rejects_bad_ranges():
    _lib, lib = _lib_()
    z = torch.zeros(64, device=DEV)
    st = torch.zeros(1, dtype=torch.int64, device=DEV)
    args = [C.c_float(LR), C.c_float(B1), C.c_float(B2), C.c_float(EPS), P(st), P(z)]
    assert lib.capgen_debug_adam(P(z), P(z), P(z), P(z), 6, *args, None, 0, 0, 0, None, None, None, None) == 1
    assert lib.capgen_debug_adam(P(z), P(z), P(z), P(z), 8, *args, None, 0, 0, 5, None, None, None, None) == 1
    assert st.item() == 0


@gpu
@pytest.mark.parametrize("n,shift", [(4100, 0), (4099, 0), (4100, 1)])
def test_to_bf16(n, shift):
    """the 4-per-lane form (n % 4 == 0, aligned), the scalar form (n = 4099), and the scalar form an
    8-byte-misaligned destination forces"""
    src = torch.randn(n, generator=gen(n + shift)) * 100
    src[:4] = torch.tensor([0.0, -0.0, 1.00390625, 1.01171875])  # two round-to-even ties
    buf = torch.full((n + shift + 4,), 7.0, dtype=torch.bfloat16, device=DEV)
    dst = buf[shift:]
    sd = dev(src)
    call("capgen_debug_to_bf16", P(sd), P(dst), n, None)
    assert_same(dst[:n], src.bfloat16(), "to_bf16")
    assert (buf[:shift] == 7.0).all() and (dst[n:] == 7.0).all()


@gpu
@pytest.mark.parametrize("n", [1, 300_001])
def test_arena_checksum(n):
    x = torch.randn(n, generator=gen(n))

    def ref(t):
        bits = t.numpy().view(np.uint32).tolist()
        return sum(b * (2 * i + 1) for i, b in enumerate(bits)) & M64

    def run(t):
        out = C.c_uint64(0)
        td = dev(t)
        call("capgen_debug_arena_checksum", P(td), n, C.byref(out), None)
        return out.value

    assert run(x) == ref(x)
    if n > 1:
        y = x.clone()
        y[[10, 200_000]] = x[[200_000, 10]]
        assert run(y) == ref(y) != ref(x), "the checksum must depend on the order"


# ---- greedy / beam selection -------------------------------------------------------------------------
SPECIAL = [0, 15, 16, 255, 256, 511, 512, -9, -1]
SEL_VS = [16, 520, 1000, 10000, 10248, 16384]  # 10248: past the 256x40 / 512x20 register forms
MARGIN = 1e-4
SOFT_PREV = 0.15


def sel_logits(rows, V, n_plant, seed):
    """logits 2 N(0,1); in each row r, n_plant columns -- 4 to 7 of the special ones (row-dependent), then
    columns spread over the row -- are set to max(all) + 1 - 0.125 n - 0.03125 (r % 3)"""
    g = gen(seed)
    x = 2 * torch.randn(rows, V, generator=g)
    top = x.max().item()
    for r in range(rows):
        sp = list(dict.fromkeys(c for c in (c if c >= 0 else V + c for c in SPECIAL) if 0 <= c < V))
        take = 4 + (r + seed) % 4
        start = (r * 2) % len(sp)
        cols = list(dict.fromkeys((sp[start:] + sp[:start])[:take]))
        c, stepc = (5 + 3 * r) % V, max(1, V // (n_plant + 3))
        while len(cols) < min(n_plant, V):
            if c not in cols:
                cols.append(c)
            c = (c + stepc) % V if (c + stepc) % V not in cols else (c + 1) % V
        for n, col in enumerate(cols):
            x[r, col] = top + 1 - 0.125 * n - 0.03125 * (r % 3)
    return x.float()


def sel_scores(x, prev, logsm):
    x64 = x.double()
    lse = torch.logsumexp(x64, 1, keepdim=True)
    s = x64 - lse if logsm else torch.exp(x64 - lse)
    return s + (0 if prev is None else prev.double().unsqueeze(1))


def beam_ref(x, prev, k_in, B, V, k, logsm):
    """per image the k best of (score desc, flat index j * V + v asc): a stable sort's first k; also the
    smallest gap between consecutive scores of ranks 1 .. k + 1"""
    s = sel_scores(x, prev, logsm).view(k_in, B, V)
    prob = torch.zeros(k, B, dtype=torch.float64)
    src = torch.zeros(k, B, dtype=torch.int32)
    tok = torch.zeros(k, B, dtype=torch.int32)
    gap = float("inf")
    for i in range(B):
        flat = s[:, i, :].reshape(-1).numpy()
        order = np.argsort(-flat, kind="stable")[:k + 1]
        best = flat[order]
        if len(best) > 1:
            gap = min(gap, float(np.min(best[:-1] - best[1:])))
        prob[:, i] = torch.from_numpy(best[:k].copy())
        src[:, i] = torch.from_numpy((order[:k] // V).astype(np.int32))
        tok[:, i] = torch.from_numpy((order[:k] % V).astype(np.int32))
    return prob, src, tok, gap


@functools.lru_cache(maxsize=None)
def sel_case(V, k, k_in, logsm, B=2):
    """a case whose reference has the margin: the fixed seeds are tried in order until the construction
    gives one (the condition itself is asserted by the caller)"""
    rows = k_in * B
    for attempt in range(200):
        seed = 100_003 * attempt + 17 * V + 5 * k + k_in + 2 * logsm
        x = sel_logits(rows, V, k + 2, seed)
        g = gen(seed + 1)
        # distinct prev per row; spread so that the beams interleave in the top k
        prev = (-0.0437 * (torch.arange(rows) // B) - 0.0113 * torch.rand(rows, generator=g)).float()
        if not logsm:
            prev = prev * SOFT_PREV  # (softmax scores lie in (0, 1): a spread of the same order)
        ref = beam_ref(x, prev, k_in, B, V, k, logsm)
        if ref[3] >= 2 * MARGIN:
            return x, prev, ref
    raise AssertionError(f"no draw with the margin for V={V} k={k} k_in={k_in} logsm={logsm}")


def sel_cases(V, k):
    for k_in in sorted({1, k}):
        if k_in * k > 256 or k > k_in * V:
            continue
        for logsm in (0, 1):
            yield k_in, logsm


def check_beam(tag, ref, out_prob, out_src, out_tok):
    prob, src, tok, gap = ref
    assert gap >= MARGIN, tag + f": the reference's own margin is {gap:.2e}"  # (a condition on the inputs)
    assert_same(out_src, src.reshape(-1), tag + " source beams")
    assert_same(out_tok, tok.reshape(-1), tag + " tokens")
    err = (out_prob.cpu().double() - prob.reshape(-1)).abs().max().item()
    assert err <= 1e-5, tag + f": scores off by {err:.2e}"


def run_beam_topk(x, stats, prev, k_in, B, V, k, logsm):
    cv = torch.zeros(k_in * B * k, device=DEV)
    ci = torch.zeros(k_in * B * k, dtype=torch.int32, device=DEV)
    op = torch.full((k * B + 1,), 7.0, device=DEV)
    os_ = torch.full((k * B + 1,), -7, dtype=torch.int32, device=DEV)
    ot = torch.full((k * B + 1,), -7, dtype=torch.int32, device=DEV)
    xd, sd, pd = dev(x), dev(stats), dev(prev)
    call("capgen_debug_beam_step_topk", P(xd), P(sd), P(pd), k_in, B, V, k, logsm, P(cv), P(ci), P(op), P(os_), P(ot),
         None)
    assert op[k * B].item() == 7.0 and os_[k * B].item() == -7 and ot[k * B].item() == -7
    return op[:k * B], os_[:k * B], ot[:k * B]


KS = [1, 3, 5, 8, 16]


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("V", SEL_VS + [20000])
def test_beam_step_topk_full_row(V, k):
    """beam_row_topk_kernel<KM, NV, NT>: KM = 4 (k <= 4), 5, 8, 16; <KM, 20, 512> (V <= 10240, KM <= 8),
    <KM, 40> (KM = 16, V <= 10240), <KM, 0> (V > 10240); then beam_merge_kernel"""
    B = 2
    for k_in, logsm in sel_cases(V, k):
        x, prev, ref = sel_case(V, k, k_in, logsm)
        out = run_beam_topk(x, None, prev, k_in, B, V, k, logsm)
        check_beam(f"V={V} k={k} k_in={k_in} logsm={logsm}", ref, *out)
    # prev is optional (the first step): scores are the row's own
    x, _, _ = sel_case(V, k, 1, 1)
    ref = beam_ref(x, None, 1, B, V, k, 1)
    check_beam(f"V={V} k={k} no prev", ref, *run_beam_topk(x, None, None, 1, B, V, k, 1))


def dec_stats_of(x):
    st, _ = slab_stats(x)
    return st.contiguous()


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("V", SEL_VS)
def test_beam_step_topk_slab(V, k):
    """slab_row_topk_kernel<KM> (KM = 4, 5, 8, 16) + beam_merge_kernel, from the decode epilogue's stats"""
    B = 2
    for k_in, logsm in sel_cases(V, k):
        x, prev, ref = sel_case(V, k, k_in, logsm)
        out = run_beam_topk(x, dec_stats_of(x), prev, k_in, B, V, k, logsm)
        check_beam(f"V={V} k={k} k_in={k_in} logsm={logsm}", ref, *out)


def run_slab_step(x, prev, k_in, B, V, k, logsm, t, Tw=7, Tc=6):
    """beam_slab_step with distinct contents per source row; returns the outputs and checks the gathers"""
    R, Rs = k * B, max(k, k_in) * B  # rows written / rows a source index can name
    g = gen(V + k + t)
    seq_src = torch.randint(100, 10_000, (Rs, Tw), generator=g, dtype=torch.int64)
    ids_src = torch.randint(100, 10_000, (Rs, Tc), generator=g, dtype=torch.int32)
    kv_src = torch.randint(100, 10_000, (Rs, Tc), generator=g, dtype=torch.int32)
    seq_dst = torch.full((R + 1, Tw), -7, dtype=torch.int64, device=DEV)
    ids_dst = torch.full((R + 1, Tc), -7, dtype=torch.int32, device=DEV)
    kv_dst = torch.full((R + 1, Tc), -7, dtype=torch.int32, device=DEV)
    op = torch.full((R + 1,), 7.0, device=DEV)
    os_ = torch.full((R + 1,), -7, dtype=torch.int32, device=DEV)
    ot = torch.full((R + 1,), -7, dtype=torch.int32, device=DEV)
    xd, sd, pd = dev(x), dev(dec_stats_of(x)), dev(prev)
    ss, is_, ks = dev(seq_src), dev(ids_src), dev(kv_src)
    call("capgen_debug_beam_slab_step", P(xd), P(sd), P(pd), k_in, B, V, k, logsm, P(op), P(os_), P(ot), P(ss),
         P(seq_dst), Tw, P(is_), P(ids_dst), P(ks), P(kv_dst), Tc, t, None)
    assert op[R].item() == 7.0 and os_[R].item() == -7 and ot[R].item() == -7
    assert (seq_dst[R] == -7).all() and (ids_dst[R] == -7).all() and (kv_dst[R] == -7).all()
    src, tok = os_[:R].cpu(), ot[:R].cpu()
    e_seq, e_ids, e_kv = seq_src[:R].clone(), ids_src[:R].clone(), kv_src[:R].clone()
    for j in range(k):
        for i in range(B):
            r, srow = j * B + i, int(src[j * B + i]) * B + i
            e_seq[r] = seq_src[srow]
            e_seq[r, t + 1] = int(tok[r])
            e_ids[r] = ids_src[srow]
            e_ids[r, t + 1] = int(tok[r])
            e_kv[r] = 0
            e_kv[r, :t + 1] = kv_src[srow, :t + 1]
            e_kv[r, t + 1] = r
    assert_same(seq_dst[:R], e_seq, "sequences")
    assert_same(ids_dst[:R], e_ids, "ids")
    assert_same(kv_dst[:R], e_kv, "K/V row table")
    assert torch.equal(ss.cpu(), seq_src) and torch.equal(is_.cpu(), ids_src) and torch.equal(ks.cpu(), kv_src)
    return op[:R], os_[:R], ot[:R]


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("V", SEL_VS)
def test_beam_slab_step(V, k):
    """beam_slab_step_kernel<KM>: the slab selection, the merge and the gathers in one launch"""
    B = 2
    for n, (k_in, logsm) in enumerate(sel_cases(V, k)):
        x, prev, ref = sel_case(V, k, k_in, logsm)
        out = run_slab_step(x, prev, k_in, B, V, k, logsm, t=(0, 3)[n % 2])
        check_beam(f"V={V} k={k} k_in={k_in} logsm={logsm}", ref, *out)
    x, prev, ref = sel_case(V, k, 1, 1)
    check_beam(f"V={V} k={k} t=3", ref, *run_slab_step(x, prev, 1, B, V, k, 1, t=3))
    check_beam(f"V={V} k={k} t=0", ref, *run_slab_step(x, prev, 1, B, V, k, 1, t=0))


def greedy_ref(x, logsm):
    s = sel_scores(x, None, logsm)
    top2 = torch.topk(s, min(2, s.shape[1]), 1).values
    gap = (top2[:, 0] - top2[:, -1]).min().item() if s.shape[1] > 1 else float("inf")
    return s.argmax(1), gap


def run_argmax(x, stats, logsm, V):
    Bn = x.shape[0]
    ids = torch.full((Bn + 1, 5), -7, dtype=torch.int64, device=DEV)
    nxt = torch.full((Bn + 1, 3), -7, dtype=torch.int32, device=DEV)
    xd, sd = dev(x), dev(stats)
    if stats is None:
        call("capgen_debug_argmax_softmax", P(xd), Bn, V, P(ids), 5, 2, P(nxt), 3, logsm, None)
    else:
        call("capgen_debug_slab_argmax", P(xd), P(sd), Bn, V, P(ids), 5, 2, P(nxt), 3, None)
    ic, nc = ids.cpu(), nxt.cpu()
    assert (ic[:, [0, 1, 3, 4]] == -7).all() and (ic[Bn] == -7).all(), "ids written outside column `col`"
    assert (nc[:, 1:] == -7).all() and (nc[Bn] == -7).all()
    assert torch.equal(ic[:Bn, 2], nc[:Bn, 0].long())
    return ic[:Bn, 2]


@gpu
@pytest.mark.parametrize("V", SEL_VS + [20000])
def test_greedy_argmax(V):
    """argmax_softmax_kernel<40> (V <= 10240) and <0>, both score forms; slab_argmax (V <= 16384);
    5 rows: the slab form takes 4 rows per workgroup"""
    x = sel_logits(5, V, 4, V)
    for logsm in (0, 1):
        ref, gap = greedy_ref(x, logsm)
        assert gap >= MARGIN, f"V={V} logsm={logsm}: the reference's own margin is {gap:.2e}"
        assert torch.equal(run_argmax(x, None, logsm, V), ref), f"V={V} logsm={logsm}"
    if V <= 16384:
        assert torch.equal(run_argmax(x, dec_stats_of(x), 1, V), greedy_ref(x, 1)[0]), f"slab V={V}"
    # next_ids is optional
    ids = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    xd = dev(x)
    call("capgen_debug_argmax_softmax", P(xd), 5, V, P(ids), 1, 0, None, 0, 1, None)
    assert torch.equal(ids.cpu(), greedy_ref(x, 1)[0])


TIE_COLS = [3, 200, 260, -1]


def tie_rows(V, rows, seed):
    """every row: bit-identical logits at columns {3, 200, 260, V - 1}, the row maximum by a margin"""
    x = 2 * torch.randn(rows, V, generator=gen(seed))
    x = x.clamp(max=4.0)
    x[:, TIE_COLS] = 6.0
    return x.float()


def tie_case(V):
    B = 2
    base = tie_rows(V, B, V)
    x = torch.cat([base, base], 0)  # row j * B + i: beam j of image i; the beams are identical
    return x, torch.tensor([-0.25, -0.5, -0.25, -0.5])


@gpu
@pytest.mark.parametrize("V", [520, 1000, 10248, 16384])
def test_greedy_ties(V):
    """'first index on ties': column 3 of {3, 200, 260, V - 1} in argmax_softmax (both score forms),
    slab_argmax and the SCST row kernel's sample"""
    x, _ = tie_case(V)
    first = torch.full((4,), 3, dtype=torch.int64)
    for logsm in (0, 1):
        assert torch.equal(run_argmax(x, None, logsm, V), first), f"argmax_softmax logsm={logsm}"
    assert torch.equal(run_argmax(x, dec_stats_of(x), 1, V), first), "slab_argmax"
    assert torch.equal(run_rl_rows(x, V)[0].cpu().long(), first), "rl_rows sample"


@gpu
@pytest.mark.parametrize("form", ["full", "slab", "step"])
@pytest.mark.parametrize("V", [520, 1000, 10248, 16384])
def test_selection_ties(V, form):
    """'(score desc, j * V + v asc)': the lowest index, then the lowest beam, wins in every beam kernel
    and for both score forms.  Two beams with identical rows and identical prev."""
    B, k_in = 2, 2
    x, prev = tie_case(V)
    cols = [c % V for c in TIE_COLS]
    stats = dec_stats_of(x)
    for logsm in (0, 1):
        for k in (1, 3, 5, 8, 16):
            exp_src, exp_tok = [], []
            s = sel_scores(x, prev, logsm).view(k_in, B, V)
            for i in range(B):
                flat = s[:, i].reshape(-1).numpy()
                order = np.argsort(-flat, kind="stable")[:k]
                exp_src.append(order // V)
                exp_tok.append(order % V)
            exp_src = torch.from_numpy(np.stack(exp_src, 1).astype(np.int32)).reshape(-1)
            exp_tok = torch.from_numpy(np.stack(exp_tok, 1).astype(np.int32)).reshape(-1)
            # (the stable sort says what the rule says: beam 0's four ties in index order, then beam 1's)
            head = [(0, c) for c in cols] + [(1, c) for c in cols]
            for sel in range(min(k, 8)):
                assert (int(exp_src[sel * B]), int(exp_tok[sel * B])) == head[sel]
            nk = min(k, 8)  # past the 8 tied candidates the order is the margin tests' business
            tag = f"V={V} k={k} logsm={logsm}"
            if form == "full":
                out = run_beam_topk(x, None, prev, k_in, B, V, k, logsm)
            elif form == "slab":
                out = run_beam_topk(x, stats, prev, k_in, B, V, k, logsm)
            else:
                out = run_slab_step(x, prev, k_in, B, V, k, logsm, t=0)
            assert_same(out[1][:nk * B], exp_src[:nk * B], f"{tag} {form} source beams")
            assert_same(out[2][:nk * B], exp_tok[:nk * B], f"{tag} {form} tokens")


# ---- SCST kernels ------------------------------------------------------------------------------------
def run_rl_rows(x, V):
    M = x.shape[0]
    sample = torch.full((M + 1,), -7, dtype=torch.int32, device=DEV)
    outs = [torch.full((M + 1,), 7.0, device=DEV) for _ in range(3)]
    xd = dev(x)
    call("capgen_debug_rl_rows", P(xd), M, V, P(sample), P(outs[0]), P(outs[1]), P(outs[2]), None)
    assert sample[M].item() == -7 and all(o[M].item() == 7.0 for o in outs)
    return sample[:M], outs[0][:M], outs[1][:M], outs[2][:M]


@gpu
@pytest.mark.parametrize("V", [8, 1000, 10000])
def test_rl_rows(V):
    x = sel_logits(5, V, 4, V + 3)
    x64 = x.double()
    lse = torch.logsumexp(x64, 1)
    lp = x64 - lse.unsqueeze(1)
    ref, gap = greedy_ref(x, 1)
    assert gap >= MARGIN
    ent = -(torch.exp(lp) * lp).sum(1)
    sample, g_lse, g_lp, g_ent = run_rl_rows(x, V)
    assert torch.equal(sample.cpu().long(), ref)
    assert_close(g_lse, lse, F32, "lse")
    assert_close(g_lp, lp[torch.arange(5), ref], F32, "logp[sample]")
    assert_close(g_ent, ent, F32, "entropy")


def rl_mask(sample):
    """mask[b, t] = 1 at t = 0, else sample[b, t-1] > 0 (rl.hip header)"""
    m = torch.ones_like(sample, dtype=torch.float64)
    m[:, 1:] = (sample[:, :-1] > 0).double()
    return m


@gpu
@pytest.mark.parametrize("L", [1, 9])
@pytest.mark.parametrize("B", [1, 3, 300])
def test_rl_image_numer_loss(B, L):
    g = gen(B * 10 + L)
    sample = torch.randint(0, 4, (B, L), generator=g, dtype=torch.int32)  # a quarter are 0: the mask bites
    if L > 1:
        sample[0, 0] = 0
    ent = torch.rand(B, L, generator=g) + 0.1
    logp = -3 * torch.rand(B, L, generator=g)
    score = 1 + 0.3 * torch.randn(B, generator=g)  # (mostly one sign: the numerator does not cancel)
    mask = rl_mask(sample)
    ent_img = torch.full((B + 1,), 7.0, device=DEV)
    scal = torch.full((3,), 7.0, device=DEV)
    sd, ed, ld, scd = dev(sample), dev(ent), dev(logp), dev(score)
    call("capgen_debug_rl_image", P(sd), P(ed), B, L, P(ent_img), P(scal), None)
    call("capgen_debug_rl_numer", P(sd), P(ld), P(scd), B, L, P(scal), None)
    assert ent_img[B].item() == 7.0 and scal[2].item() == 7.0
    assert_close(ent_img[:B], (ent.double() * mask).sum(1) / mask.sum(1), F32, "per-image entropy")
    msum = mask.sum().item()
    numer = -(logp.double() * mask * score.double().unsqueeze(1)).sum()
    assert scal[0].item() == msum, "sum(mask) is a count"
    assert abs(scal[1].item() - numer.item()) <= 1e-5 * abs(numer.item()), (scal[1].item(), numer.item())
    struct = scal[1].item() / scal[0].item()
    for w in (0.0, 0.3, 1.0):
        lm = float("nan") if w == 1.0 else 2.5
        out = torch.full((4,), 7.0, device=DEV)
        gs = torch.full((2,), 7.0, device=DEV)
        lmd = torch.tensor([lm], device=DEV)
        call("capgen_debug_rl_loss", P(scal), P(lmd), C.c_float(w), P(out), P(gs), None)
        wf = float(np.float32(w))
        l_ = 0.0 if w == 1.0 else lm  # at w = 1 the LM loss is not read
        exp = torch.tensor([(1 - wf) * l_ + wf * struct, l_, struct], dtype=torch.float64)
        assert_close(out[:3], exp, F32, f"w={w}")
        assert out[3].item() == 7.0 and gs[0].item() == 1.0 and gs[1].item() == 7.0


@gpu
@pytest.mark.parametrize("w", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("V", [8, 1000])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_rl_grad(dtype, V, w):
    """against float64 autograd of loss = (1-w) CE_mean(tgt) + w (-sum logp[sample] mask score_b / sum(mask))"""
    B, L, pad = 2, 3, 0
    M = B * L
    g = gen(V + dtype)
    x = 2 * torch.randn(M, V, generator=g)
    tgt = torch.tensor([3, pad, 5, V - 1, 2, pad], dtype=torch.int32)
    sample = torch.tensor([3, 0, 6, 1, 0, 4], dtype=torch.int32)  # row 0: sample == target; zeros mask t + 1
    score = torch.tensor([0.7, -1.3])
    wf = float(np.float32(w))
    x64 = x.double().requires_grad_(True)
    lp = x64 - torch.logsumexp(x64, 1, keepdim=True)
    kept = (tgt != pad).double()
    count = kept.sum()
    mask = rl_mask(sample.view(B, L)).reshape(-1)
    lm = -(lp[torch.arange(M), tgt.long()] * kept).sum() / count
    st = -(lp[torch.arange(M), sample.long()] * mask * score.double().repeat_interleave(L)).sum() / mask.sum()
    ((1 - wf) * lm + wf * st).backward()
    lse = torch.logsumexp(x.double(), 1).float()
    dl = torch.full((M * V + 8,), 7.0, dtype=TDT[dtype], device=DEV)
    xd, td, sd, ld, scd = dev(x), dev(tgt), dev(sample), dev(lse), dev(score)
    cd = torch.tensor([count.item()], device=DEV)
    scal = torch.tensor([mask.sum().item(), 0.0], device=DEV)
    call("capgen_debug_rl_grad", P(xd), P(td), P(sd), P(ld), P(scd), P(cd), P(scal), B, L, V, pad, C.c_float(w), P(dl),
         dtype, None)
    assert (dl[M * V:] == 7.0).all()
    assert_close(dl[:M * V].view(M, V), x64.grad, dtype, f"V={V} w={w}")
