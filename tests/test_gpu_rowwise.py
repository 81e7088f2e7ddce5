"""GPU: the row kernels of ssak_amd/csrc/norm_act.hip, one launch at a time, against the float64 restatement tests/rowwise_ref.py
(itself pinned to torch float64 autograd by tests/test_rowwise_ref.py), through the test-only entries ssak_debug_layernorm_fwd /
_bwd, ssak_debug_softmax_fwd / _bwd and ssak_debug_gelu.

Which dispatcher branch each case reaches (T = bf16 unless fp32 is named; "generic" = the one-row-per-wave ln_fwd_kernel<T, NCH>,
NCH = ceil(C / 512), or ln_bwd_kernel<T, NCH, VEC, PGELU, DROP> with (NCH, VEC) = (3, 4) at C = 768, else (ceil(C / 512), 8)):

* ln_fwd_rows_kernel<bf16, 3, 4, SP> / <bf16, 2, 8, SP> for every SP of LN_FWD_SPEC (C = 768 / 1024): test_ln_fwd_spec, M = 3 100
  (more rows than the 768 x 4 waves of the capped grid: waves stride with a prefetched next row); M in {1, 5, 3071, 3072, 3073,
  15968} for SP = 1, 39, 47 in test_ln_fwd_rows.
* ln_fwd_kernel<T, 1> (C = 8, 64, 512), <T, 2> (520, 768, 1024), <T, 3> (1032, 1536), both T, with every site, r_out and
  post-GELU: test_ln_fwd_generic (bf16 at 768 / 1024 with a bit set outside the list, SP = 63, and with post-GELU, which is never
  specialised); out = NULL (the dropout-only pass of the engine's projection dropout and its replay), r_out aliasing y:
  test_ln_fwd_dropout_only; fp32 at C = 1024 over the M sweep: test_ln_fwd_rows.
* ln_bwd_kernel<bf16, 3, 4 | 2, 8, false, DROP(SP), SP> for every SP of LN_BWD_SPEC: test_ln_bwd_spec (M = 3 100, dy column sum
  whenever dy is written, the queued second stage on every other case); M sweep for SP = 3, 52: test_ln_bwd_rows.
* ln_bwd_kernel<T, N, V, PGELU, DROP> generic: (1, 8) at C = 8, 64, 512; (2, 8) at 520 (and 1024 fp32); (3, 8) at 1032, 1536;
  (3, 4) at 768 -- each with DROP = false (no site), DROP = true (every site, g2, g_res, dy) and PGELU (with and without
  dropout): test_ln_bwd_generic.  bf16 (3, 4) / (2, 8) at 768 / 1024 with DROP = false are never launched (every bit set without
  dropout is specialised there); with DROP they are reached by SP = 63.
* reduce_jobs_kernel, launched directly by k_reduce and from the queue by k_reduce_flush: every backward case (alternating), the
  two bit-identical to each other in test_ln_bwd_deterministic; the bound of its unrolled loop (241, 256, 257 partial rows) and a
  partly filled column block (C = 72), on both paths: test_ln_bwd_reduce_unroll_edges.
* softmax_fwd_kernel / softmax_bwd_kernel<T, 1 | 2 | 3> (ld <= 512, <= 1024, <= 1536), both T: test_softmax.

Data: every 7 rows cycle through a constant row (its output must be beta), a row of std ~3e-3 (variance near eps = 1e-5),
a row with mean ~68 and spread ~2 in values bf16 holds exactly, and four N(0.3, 1.5) rows.  Dropout p in {0.1, 0.5}; the sites'
masks come from oracle.dropout_hash (pinned to the device by test_gpu_dropout.py).

Bars (u = 2^-24, the fp32 unit roundoff; eps_st = 2^-8 for bf16 storage -- half a bf16 ulp is at most 2^-8 relative -- and
2^-22 for fp32 storage):

* Dropout: a dropped position is exactly 0 in r_out, out, dr and dy (and in Pd); kept positions carry the scale through the
  value bars below (a missing 1 / (1 - p) is a 10 % error).
* r_out within one storage ulp of the float64 composition, plus u times its terms (the fp32 add before the rounding).
* mean within 4e-6 mean|r| (a 64-lane DPP tree over <= 24 sequential terms: ~30 u relative); rstd within 1e-5 relative of the
  float64 statistics of the STORED r.  A variance divided by C - 1 moves rstd by 1 / 2C >= 3.3e-4 (C <= 1536; still > 1e-4 on
  the near-eps rows), eps outside the root moves it by > 20 % on the near-eps rows: both fail.
* out: |got - ref| <= eps_st |ref| + floor, floor = 1e-5 (|xhat gamma| + |beta|) + 4e-6 rstd mean|r| |gamma| (the fp32
  statistics; the second term is the cancellation in r - mean on the large-mean rows), times the post-dropout scale.
* dr, dy (the reference runs on the kernel's inputs and the same saved mean / rstd, so forward errors do not enter):
  |got - ref| <= eps_st |ref| + 2^-16 rstd max_row|a gamma| (1 + |xhat|) + 2^-23 |g_res| (fp32 sums of C terms in the two row
  reductions, then the cancellation a gamma - mean - xhat mean(..)), times the site scales.
* dgamma, dbeta, dy column sum are added onto non-zero starting values: |got - start - ref| <= 1e-5 sum|terms| + 2^-23
  (|start| + |ref|).
* Softmax: P within one bf16 ulp (fp32: 1e-5 relative) of float64; masked keys and pad columns [cols, ld) exactly 0, a row
  with no valid key all 0; rows sum to 1 within 2^-8 (fp32: 1e-5).  dS within one bf16 ulp (fp32: 1e-5 relative) plus
  4e-6 P (|dP| + sum|P dP|) for the cancellation dP - dot.
* GELU over [-12, 12] (clamp points +-6 and their neighbours included): bf16 fit |gelu - x Phi(x)| <= 1.65e-5 |x| + 2^-22 |gelu|
  and |gelu' - (Phi(x) + x phi(x))| <= 1.65e-5 + 2^-20, and within 1e-6 of the float64 restatement of the fit; fp32 (erff) within
  1e-6 |x| and 1e-6.
* Two launches are bit-identical, and so are the queued and the direct column sums (reduce_jobs_kernel either way: the same
  summation order, whatever else shares the launch).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rowwise_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
SEED = 0x5EED00001234ABCD
PRE, MID, POST = 19, 2, 5  # site ids (any distinct ones: the engine's hidden-dropout, encoder-input and a spare id)
EPS = 1e-5
U = 2.0 ** -24
GENERIC_C = (8, 64, 512, 520, 768, 1024, 1032, 1536)
ROWS = (1, 5, 3071, 3072, 3073, 15968)


def _hip():
    import ssak_amd.hip as hip
    return hip


def _eps_st(bf):
    return 2.0 ** -8 if bf else 2.0 ** -22


def _ulp_st(x, bf):
    return RR.bf16_ulp(x) if bf else 2.0 ** -23 * np.abs(x) + 1e-45


def _dev(a, dt):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).to(dt).contiguous()


def _host(t):
    return None if t is None else t.double().cpu().numpy()


def _nan(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


def _rows(rng, M, C, kind_of_row=True):
    """[M, C] float64 rows cycling through the data kinds (see the module docstring)."""
    x = rng.standard_normal((M, C)) * 1.5 + 0.3
    if kind_of_row:
        i = np.arange(M)
        const = i % 7 == 0
        x[const] = ((i[const] % 5) - 2)[:, None] / 4.0
        near = i % 7 == 1
        x[near] = rng.standard_normal((int(near.sum()), C)) * 3e-3 + 1e-3
        big = i % 7 == 2
        x[big] = 64.0 + 0.5 * rng.integers(0, 16, (int(big.sum()), C))
    return x


def _operands(rng, M, C, has_y, has_res, bf):
    """(y, res) rounded to the storage type: with both, the branch y carries the small part (0 on constant rows, ~2e-3 on the
    near-eps rows) and the residual the rest."""
    x = _rows(rng, M, C)
    if has_y and has_res:
        i = np.arange(M) % 7
        y = rng.standard_normal((M, C)) * 0.7
        y[i == 0] = 0.0
        y[i == 1] *= 2e-3
        y[i == 2] = 0.5 * rng.integers(-2, 3, (int((i == 2).sum()), C))
        return RR.round_to(y, bf), RR.round_to(x, bf)
    return (RR.round_to(x, bf), None) if has_y else (None, RR.round_to(x, bf))


def _affine(rng, C):
    return (1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32).astype(np.float64), \
        (0.1 * rng.standard_normal(C)).astype(np.float32).astype(np.float64)


def _check(name, got, ref, bar):
    assert got.shape == ref.shape, name
    assert np.isfinite(got).all(), f"{name}: non-finite"
    err = np.abs(got - ref)
    bad = err > bar
    if bad.any():
        k = np.unravel_index(np.argmax(err - bar), err.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} outside the bar; worst at {k}: got {got[k]!r} "
                             f"ref {ref[k]!r} bar {bar[k] if np.ndim(bar) else bar!r}")


def _zeros_where_dropped(name, got, keep):
    if keep is not None:
        assert (got[~keep] == 0).all(), f"{name}: {int((got[~keep] != 0).sum())} dropped positions are not 0"


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def run_ln_fwd(dt, M, C, *, y=True, res=True, pre=0.0, mid=0.0, post=0.0, rout=True, out=True, gelu=False, alias=False, seed=SEED,
               rng_seed=0):
    hip = _hip()
    bf = dt == BF
    rng = np.random.default_rng(rng_seed)
    Y, R = _operands(rng, M, C, y, res, bf)
    gamma, beta = _affine(rng, C)
    ty, tres = (None if Y is None else _dev(Y, dt)), (None if R is None else _dev(R, dt))
    tg, tb = _dev(gamma, F32), _dev(beta, F32)
    r_out = ty if alias else (_nan((M, C), dt) if rout else None)
    o = _nan((M, C), dt) if out else None
    mean, rstd = (_nan((M,), F32), _nan((M,), F32)) if out else (None, None)
    hip.debug_layernorm_fwd(ty, tres, tg if out else None, tb if out else None, r_out, o, mean, rstd, eps=EPS, seed=seed,
                            pre=(PRE, pre), mid=(MID, mid), post=(POST, post), post_gelu=gelu)
    torch.cuda.synchronize()
    sites = dict(seed=seed, pre=(PRE, pre), mid=(MID, mid))
    comp = RR.ln_fwd(Y, R, gamma, beta, eps=EPS, want_out=False, **sites)
    sp, sm = RR.site_mask(seed, (PRE, pre), (M, C))[1], RR.site_mask(seed, (MID, mid), (M, C))[1]
    if r_out is not None:
        got_r = _host(r_out)
        terms = (np.abs(Y) * sp if Y is not None else 0.0) + (np.abs(R) if R is not None else 0.0)
        _check("r_out", got_r, comp["r"], _ulp_st(comp["r"], bf) + 2 * U * terms * sm)
        _zeros_where_dropped("r_out (sum dropout)", got_r, comp["keep_mid"])
        if R is None:
            _zeros_where_dropped("r_out (pre dropout)", got_r, comp["keep_pre"])
        r = got_r
    else:
        r = comp["r"]
    if not out:
        return
    m_ref, s_ref = RR.ln_stats(r, EPS)
    got_m, got_s = _host(mean), _host(rstd)
    _check("mean", got_m, m_ref, 4e-6 * np.abs(r).mean(axis=1) + 1e-30)
    _check("rstd", got_s, s_ref, 1e-5 * s_ref)
    gl = RR.gelu_forms(bf)[0]
    f = RR.ln_fwd(None, r, gamma, beta, eps=EPS, seed=seed, post=(POST, post), post_gelu=gelu, gelu=gl)
    xg = np.abs((r - m_ref[:, None]) * s_ref[:, None] * gamma)
    sq = RR.site_mask(seed, (POST, post), (M, C))[1]
    floor = (1e-5 * (xg + np.abs(beta)) + 4e-6 * (s_ref * np.abs(r).mean(axis=1))[:, None] * np.abs(gamma)) * 1.2 * sq
    got_o = _host(o)
    _check("out", got_o, f["out"], _eps_st(bf) * np.abs(f["out"]) + floor)
    _zeros_where_dropped("out (post dropout)", got_o, f["keep_post"])
    # constant rows (no sum-dropout to break them, no GELU, no post-dropout): the output is beta (up to the storage rounding and
    # the last bit of the fp32 mean times rstd = 1 / sqrt(eps))
    if not mid and not gelu and not post:
        const = np.ptp(r, axis=1) == 0
        if const.any():
            c = r[const, :1]
            _check("mean (constant rows)", got_m[const], c[:, 0], 2 * U * np.abs(c[:, 0]))
            _check("out (constant rows)", got_o[const], np.broadcast_to(beta, got_o[const].shape),
                   _eps_st(bf) * np.abs(beta) + 4 * U * np.abs(c) * s_ref[const, None] * np.abs(gamma) + 1e-30)


def _fwd_bits(sp):
    return dict(y=bool(sp & RR.FWD_Y), res=bool(sp & RR.FWD_RES), rout=bool(sp & RR.FWD_ROUT))


def _fwd_cases():
    for sp in RR.LN_FWD_SPECS:
        for C in (768, 1024):
            ps = (0.1, 0.5) if sp & (RR.FWD_PRE | RR.FWD_MID | RR.FWD_POST) else (0.0,)
            for p in ps:
                yield pytest.param(sp, C, p, id=f"spec{sp}-C{C}-p{p}")


@pytest.mark.parametrize("spec,C,p", list(_fwd_cases()))
def test_ln_fwd_spec(spec, C, p):
    """Every specialised forward instantiation (bf16, C = 768 / 1024) on more rows than its capped grid has waves."""
    run_ln_fwd(BF, 3100, C, pre=p if spec & RR.FWD_PRE else 0.0, mid=p if spec & RR.FWD_MID else 0.0,
               post=p if spec & RR.FWD_POST else 0.0, rng_seed=spec * 7 + C, **_fwd_bits(spec))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", GENERIC_C)
@pytest.mark.parametrize("variant", ["all_sites", "post_gelu", "gelu_drop", "plain"])
def test_ln_fwd_generic(dt, C, variant):
    """The one-row-per-wave forward at every NCH, both storage types: every site with r_out (bf16 bit set 63 at C = 768 / 1024,
    outside the specialised list), post-GELU alone (the XLSR conv-layer LN, C = 512) and with post-dropout, and a plain LN."""
    kw = dict(all_sites=dict(pre=0.1, mid=0.5, post=0.1), post_gelu=dict(res=False, rout=False, gelu=True),
              gelu_drop=dict(res=False, rout=False, gelu=True, post=0.5), plain=dict(y=False, rout=False))[variant]
    run_ln_fwd(dt, 517, C, rng_seed=C + len(variant), **kw)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [64, 768, 1024])
@pytest.mark.parametrize("alias", [True, False], ids=["r_out=y", "r_out"])
def test_ln_fwd_dropout_only(dt, C, alias):
    """out = NULL: the engine's projection-dropout pass and its backward replay (one site, r_out aliasing y), no statistics."""
    run_ln_fwd(dt, 3073, C, res=False, pre=0.1, out=False, alias=alias, rng_seed=C)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("case", ["bf16-spec47-C768", "bf16-spec39-C1024", "bf16-spec1-C1024", "fp32-C1024"])
def test_ln_fwd_rows(case, M):
    """Row counts around the capped grid (768 workgroups x 4 waves = 3 072 rows) and the train shape 15 968 = 32 x 499."""
    if case.startswith("fp32"):
        run_ln_fwd(F32, M, 1024, pre=0.1, mid=0.1, post=0.1, rng_seed=M)
        return
    sp, C = int(case.split("spec")[1].split("-")[0]), int(case.split("C")[1])
    run_ln_fwd(BF, M, C, pre=0.1 if sp & RR.FWD_PRE else 0.0, mid=0.1 if sp & RR.FWD_MID else 0.0, rng_seed=M, **_fwd_bits(sp))


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def run_ln_bwd(dt, M, C, *, dy=True, pre=0.0, mid=0.0, post=0.0, g2=True, gres=True, pgelu=False, colsum=None, queued=False,
               seed=SEED, rng_seed=0, repeat=False):
    """One backward launch checked against the reference; returns the outputs (host arrays) for the determinism test."""
    hip = _hip()
    bf = dt == BF
    colsum = dy if colsum is None else colsum
    rng = np.random.default_rng(rng_seed)
    R = RR.round_to(_rows(rng, M, C), bf)
    mean, rstd = (v.astype(np.float32).astype(np.float64) for v in RR.ln_stats(R, EPS))
    gamma, beta = _affine(rng, C)
    G1 = RR.round_to(rng.standard_normal((M, C)), bf)
    G2 = RR.round_to(rng.standard_normal((M, C)), bf) if g2 else None
    GR = RR.round_to(rng.standard_normal((M, C)) * 0.5, bf) if gres else None
    start = [rng.standard_normal(C).astype(np.float32).astype(np.float64) for _ in range(3)]
    t = dict(g1=_dev(G1, dt), g2=None if G2 is None else _dev(G2, dt), r=_dev(R, dt), mean=_dev(mean, F32), rstd=_dev(rstd, F32),
             gamma=_dev(gamma, F32), g_res=None if GR is None else _dev(GR, dt), beta=_dev(beta, F32) if pgelu else None)

    def launch(q):
        outs = dict(dr=_nan((M, C), dt), dy=_nan((M, C), dt) if dy else None, dgamma=_dev(start[0], F32), dbeta=_dev(start[1], F32),
                    dy_colsum=_dev(start[2], F32) if colsum else None)
        hip.debug_layernorm_bwd(t["g1"], t["g2"], t["r"], t["mean"], t["rstd"], t["gamma"], t["g_res"], outs["dr"], outs["dy"],
                                outs["dgamma"], outs["dbeta"], outs["dy_colsum"], t["beta"], seed=seed, pre=(PRE, pre), mid=(MID, mid),
                                post=(POST, post), queued=q)
        torch.cuda.synchronize()
        return {k: _host(v) for k, v in outs.items()}

    got = launch(queued)
    ref = RR.ln_bwd(G1, G2, R, mean, rstd, gamma, GR, seed=seed, pre=(PRE, pre), mid=(MID, mid), post=(POST, post),
                    gelu_beta=beta if pgelu else None, gelu_grad=RR.gelu_forms(bf)[1])
    xh = np.abs((R - mean[:, None]) * rstd[:, None])
    sm, sp = RR.site_mask(seed, (MID, mid), (M, C))[1], RR.site_mask(seed, (PRE, pre), (M, C))[1]
    floor = (2.0 ** -16 * (rstd * np.abs(ref["a"] * gamma).max(axis=1))[:, None] * (1 + xh)
             + (2.0 ** -23 * np.abs(GR) if GR is not None else 0.0)) * sm
    _check("dr", got["dr"], ref["dr"], _eps_st(bf) * np.abs(ref["dr"]) + floor)
    _zeros_where_dropped("dr (sum dropout)", got["dr"], ref["keep_mid"])
    if dy:
        _check("dy", got["dy"], ref["dy"], _eps_st(bf) * np.abs(ref["dy"]) + floor * sp)
        _zeros_where_dropped("dy (sum dropout)", got["dy"], ref["keep_mid"])
        _zeros_where_dropped("dy (pre dropout)", got["dy"], ref["keep_pre"])
    for k, s0 in zip(("dgamma", "dbeta", "dy_colsum"), start):
        if got[k] is None:
            continue
        _check(k, got[k] - s0, ref[k], 1e-5 * ref["terms"][k] + 2.0 ** -23 * (np.abs(s0) + np.abs(ref[k])))
    if repeat:
        return got, launch(queued), launch(not queued)
    return got


def _bwd_kw(sp, p):
    return dict(dy=bool(sp & RR.BWD_DY), pre=p if sp & RR.BWD_PRE else 0.0, mid=p if sp & RR.BWD_MID else 0.0,
                post=p if sp & RR.BWD_POST else 0.0, g2=bool(sp & RR.BWD_G2), gres=bool(sp & RR.BWD_GRES))


def _bwd_cases():
    n = 0
    for sp in RR.LN_BWD_SPECS:
        for C in (768, 1024):
            for p in ((0.1, 0.5) if sp & (RR.BWD_PRE | RR.BWD_MID | RR.BWD_POST) else (0.0,)):
                n += 1
                yield pytest.param(sp, C, p, n % 2 == 0, id=f"spec{sp}-C{C}-p{p}" + ("-queued" if n % 2 == 0 else ""))


@pytest.mark.parametrize("spec,C,p,queued", list(_bwd_cases()))
def test_ln_bwd_spec(spec, C, p, queued):
    """Every specialised backward instantiation (bf16, C = 768 / 1024) with its operands, sites and column sums."""
    run_ln_bwd(BF, 3100, C, queued=queued, rng_seed=spec * 11 + C, **_bwd_kw(spec, p))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", GENERIC_C)
@pytest.mark.parametrize("variant", ["all_sites", "no_drop", "pgelu", "pgelu_drop"])
def test_ln_bwd_generic(dt, C, variant):
    """The generic backward at every (NCH, VEC) x {no dropout, dropout, PGELU}, both storage types."""
    kw = dict(all_sites=dict(pre=0.5, mid=0.1, post=0.1), no_drop=dict(), pgelu=dict(dy=False, g2=False, gres=False, pgelu=True),
              pgelu_drop=dict(dy=True, g2=False, gres=False, pgelu=True, pre=0.1, post=0.5))[variant]
    run_ln_bwd(dt, 517, C, queued=C % 3 == 0, rng_seed=C + 3 * len(variant), **kw)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("case", ["bf16-spec3-C1024", "bf16-spec52-C768", "fp32-C768"])
def test_ln_bwd_rows(case, M):
    """Row counts around the capped grid and the train shape, on the strided rows with prefetch."""
    if case.startswith("fp32"):
        run_ln_bwd(F32, M, 768, pre=0.1, mid=0.1, post=0.1, rng_seed=M)
        return
    sp, C = int(case.split("spec")[1].split("-")[0]), int(case.split("C")[1])
    run_ln_bwd(BF, M, C, rng_seed=M, **_bwd_kw(sp, 0.1))


@pytest.mark.parametrize("case", ["bf16-spec51-C1024", "bf16-spec36-C768", "bf16-generic-C512", "fp32-C1536"])
def test_ln_bwd_deterministic(case):
    """Two launches are bit-identical, and the queued second stage (ReduceSink + k_reduce_flush, the engine's path) equals the
    direct launch of reduce_jobs_kernel bit for bit."""
    if case.startswith("fp32"):
        a, b, c = run_ln_bwd(F32, 6000, 1536, pre=0.1, mid=0.1, post=0.1, repeat=True)
    elif "generic" in case:
        a, b, c = run_ln_bwd(BF, 7001, 512, pre=0.1, post=0.1, repeat=True)
    else:
        sp, C = int(case.split("spec")[1].split("-")[0]), int(case.split("C")[1])
        a, b, c = run_ln_bwd(BF, 7001, C, repeat=True, **_bwd_kw(sp, 0.1))
    for k in a:
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), f"{k}: two launches differ"
            assert np.array_equal(a[k], c[k]), f"{k}: queued and direct second stages differ"


@pytest.mark.parametrize("C", [64, 72])
@pytest.mark.parametrize("M", [964, 1024, 1028])
def test_ln_bwd_reduce_unroll_edges(M, C):
    """The second stage's sixteen-loads-in-flight loop runs while k + 240 < slots, k = ry, ry + 256, ...: M = 964, 1024, 1028 rows
    are 241, 256, 257 partial rows -- at 241 only slot group 0 enters the unrolled loop, 256 and 257 sit either side of its tail
    (at 257 group 0 has one slot left over for the scalar loop).  C = 72: the second column block holds 8 of its 64 columns.
    Against the reference with the usual bars, and direct against queued bit for bit."""
    a, b, c = run_ln_bwd(BF, M, C, pre=0.1, rng_seed=M + C, repeat=True)
    for k in a:
        assert a[k] is not None, k
        assert np.array_equal(a[k], b[k]), f"{k}: two launches differ"
        assert np.array_equal(a[k], c[k]), f"{k}: queued and direct second stages differ"


# ------------------------------------------------------------------------------------------------ softmax
def _softmax_cases():
    for cols in (1, 7, 64, 499, 513, 1500, 1536):
        ld0 = -(-cols // 8) * 8
        for ld in sorted({ld0, min(1536, ld0 + 24)}):
            yield cols, ld


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cols,ld", list(_softmax_cases()))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_softmax(dt, cols, ld, p):
    """Forward and backward of the unfused attention softmax: ragged key lengths per utterance (some cols, 1, more than cols and
    0), rows_per_batch = nh F as the engine passes it, pad columns, dropout."""
    hip = _hip()
    bf = dt == BF
    rng = np.random.default_rng(cols * 31 + ld + int(p * 10))
    nh, F = 2, min(cols, 40)
    klens = np.array([cols, 1, cols + 9, max(1, cols - cols // 3), 0], dtype=np.int32)
    rows = len(klens) * nh * F
    S = RR.round_to(rng.standard_normal((rows, ld)) * 3, bf)
    S[:, cols:] = 1e4 if not bf else 256.0  # pad columns hold garbage the kernel must not read as keys
    dPd = RR.round_to(rng.standard_normal((rows, ld)), bf)
    tS, tk = _dev(S, dt), torch.tensor(klens, device=DEV)
    P, Pd = _nan((rows, ld), dt), (_nan((rows, ld), dt) if p else None)
    hip.debug_softmax_fwd(tS, P, Pd, tk, cols, nh * F, seed=SEED, site=PRE, p=p)
    torch.cuda.synchronize()
    ref = RR.softmax_fwd(S, cols, klens, nh * F, seed=SEED, site=(PRE, p))
    gP = _host(P)
    bar = RR.bf16_ulp(ref["P"]) if bf else 1e-5 * ref["P"]
    _check("P", gP, ref["P"], np.where(ref["P"] > 0, bar, 0.0))
    assert (gP[~ref["valid"]] == 0).all(), "masked keys / pad columns / key-less rows are not 0"
    live = ref["valid"].any(axis=1)
    assert np.abs(gP[live].sum(axis=1) - 1).max() <= (2.0 ** -8 if bf else 1e-5)
    if p:
        gPd = _host(Pd)
        _zeros_where_dropped("Pd", gPd, ref["keep"])
        _check("Pd", gPd, ref["Pd"], np.where(ref["Pd"] > 0, RR.bf16_ulp(ref["Pd"]) if bf else 1e-5 * ref["Pd"], 0.0))
    # backward on the stored P
    dS = _nan((rows, ld), dt)
    hip.debug_softmax_bwd(_dev(dPd, dt), P, dS, cols, seed=SEED, site=PRE, p=p)
    torch.cuda.synchronize()
    b = RR.softmax_bwd(dPd, gP, cols, seed=SEED, site=(PRE, p))
    gdS = _host(dS)
    floor = 4e-6 * gP * (np.abs(b["dP"]) + (np.abs(gP * b["dP"])).sum(axis=1, keepdims=True))
    _check("dS", gdS, b["dS"], (RR.bf16_ulp(b["dS"]) if bf else 1e-5 * np.abs(b["dS"])) + floor)
    assert (gdS[:, cols:] == 0).all() and (gdS[~live] == 0).all()


# ------------------------------------------------------------------------------------------------ GELU
def test_gelu_forms():
    """gelu_s / gelu_grad_s of both storage types over [-12, 12] with the clamp points +-6 and their fp32 neighbours."""
    hip = _hip()
    x = np.linspace(-12, 12, 480001).astype(np.float32)
    edge = np.array([6, -6], dtype=np.float32)
    x = np.concatenate([x, edge, np.nextafter(edge, 0), np.nextafter(edge, 100 * edge), [0.0]]).astype(np.float32)
    xd = x.astype(np.float64)
    tx = torch.tensor(x, device=DEV)
    yb, db = (_host(v) for v in hip.debug_gelu(tx, BF))
    yf, df = (_host(v) for v in hip.debug_gelu(tx, F32))
    torch.cuda.synchronize()
    ge, dge = RR.gelu_exact(xd), RR.gelu_grad_exact(xd)
    # bf16 engine: the logistic fit of common.h meets its stated error against the exact GELU, and is what the restatement says
    _check("gelu bf16 vs exact", yb, ge, RR.PHI_FIT_MAX_ERR * np.abs(xd) + 2.0 ** -22 * np.abs(ge))
    _check("gelu' bf16 vs exact", db, dge, np.full_like(xd, RR.PHI_FIT_MAX_ERR + 2.0 ** -20))
    _check("gelu bf16 vs fit", yb, RR.gelu_fit(xd), 1e-6 * np.abs(xd) + 2.0 ** -22 * np.abs(ge))
    _check("gelu' bf16 vs fit", db, RR.gelu_grad_fit(xd), np.full_like(xd, 1e-6))
    # fp32-exact mode: erff
    _check("gelu fp32", yf, ge, 1e-6 * np.abs(xd) + 1e-30)
    _check("gelu' fp32", df, dge, np.full_like(xd, 1e-6))
    print(f"max |Phi_fit error| on the device: {np.max(np.abs(yb - ge)[xd != 0] / np.abs(xd[xd != 0])):.3e}")
