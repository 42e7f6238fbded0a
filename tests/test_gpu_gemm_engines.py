"""GPU: every GEMM engine of csrc/gemm_route.hpp behind smi_gemm_tn / smi_gemm_tn_splitk / smi_gemm_tn_tile_stats against exact
results and elementwise fp64 bounds (tests/gemm_ref.py; its rules are tested on the CPU by tests/test_gemm_ref_cpu.py):

  (a) dyadic operands: linear epilogues bit-equal to the fp64 reference rounded once, nonlinear ones inside the bound derived from
      csrc/gemm_epi.hpp;  (b) selector operands, both orientations, every phase: out[r][c] is one operand element, bit for bit;
  (c) integer operands through split-K: every fp32 / fp16 slab and their sum exact;  (d) real-valued operands with per-row and
      per-column scales under elementwise_bound.

Every launch is pinned to its engine with the tuning switches and ASSERTED through smi_gemm_route first (a routing change fails here
instead of moving a case to another engine), starts from a NaN-filled output (read-modify-write streams: from the old values),
is repeated and must be bit-identical; every element is compared; row-major outputs also run with ldo = n + 64 and the gap must
stay NaN; bias = NULL runs wherever the header allows it."""
import ctypes as C
import functools
import types

import pytest
import torch

from tests import gemm_ref as R
from tests.tile_major import from_tile_major, to_tile_major

pytestmark = pytest.mark.gpu

RING, LONE64, LONE16, PP256, V2, V2_RESID, V2_STATS, V2_LONE128, V2_LONE160, V2_LONE192 = range(1, 11)    # SMI_GEMM_ENGINE_*
ROUTED = set()      # every engine a launch of this file was asserted to run on; checked by the last test
BLOCK = 4096        # rows per fp64 reference block


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib

    lib = _lib.load()
    _lib.check(lib.smi_init(0))
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256    # the tile counts below are sized for 256 CUs
    return lib


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _route(lib, epi_sel, m, n, k, ldo, has_bias, stats=0, ksplit=0, slab_f16=False):
    from sonar_amd import _lib

    info = _lib.GemmRouteInfo()
    _lib.check(lib.smi_gemm_route(epi_sel, m, n, k, ldo, int(has_bias), 0, 0, stats, ksplit, _lib.SMI_F16 if slab_f16 else _lib.SMI_F32, 0,
                                  C.byref(info)))
    return info


def _assert_route(info, want, tag):
    got = {f: getattr(info, f) for f in want}
    assert got == want, (tag, "routed to", {f: getattr(info, f) for f, _ in info._fields_})
    ROUTED.add(info.engine)


class Cfg:
    """one pinned engine: the tuning switches, the engine selector and layout flags of its launches, and what smi_gemm_route must
    answer for an epilogue"""

    def __init__(self, name, tuning, sel, in_tm, out_tm, expect):
        self.name, self.tuning, self.sel, self.in_tm, self.out_tm = name, tuning, sel, in_tm, out_tm
        self.expect = expect if callable(expect) else (lambda epi, e=expect: e)


def _tm(ops):
    if not hasattr(ops, "x_tm"):
        ops.x_tm, ops.w_tm = to_tile_major(ops.x), to_tile_major(ops.w)
    return ops.x_tm, ops.w_tm


def _gemm(lib, cfg, epi, ops, bias, old, pad=0, reps=2, extra_expect=None):
    """`reps` bit-identical launches of smi_gemm_tn on the engine cfg pins; returns the [m][n or n / 2] result (row-major view)"""
    from sonar_amd import _lib

    m, n, k = ops.m, ops.n, ops.k
    no = R.out_cols(epi, n)
    ldo = no + pad
    f16 = R.out_is_f16(epi)
    dtype = torch.float16 if f16 else torch.float32
    assert not (cfg.out_tm and pad) and (old is None) == (epi not in R.RMW)
    epi_sel = epi | (cfg.sel << 8) | (_lib.SMI_GEMM_IN_TM if cfg.in_tm else 0) | (_lib.SMI_GEMM_OUT_TM if cfg.out_tm else 0)
    x, w = _tm(ops) if cfg.in_tm else (ops.x, ops.w)
    tag = (cfg.name, epi, (m, n, k), "bias" if bias is not None else "no bias", f"ldo n+{pad}")
    outs = []
    with _lib.tuning(**cfg.tuning):
        info = _route(lib, epi_sel, m, n, k, ldo, bias is not None)
        _assert_route(info, dict(cfg.expect(epi), **(extra_expect or {})), tag)
        for _ in range(reps):
            if cfg.out_tm:
                out = to_tile_major(old) if old is not None else _nan((m * no,), dtype)
            else:
                out = _nan((m, ldo), dtype)
                if old is not None:
                    out[:, :no] = old
            _lib.check(lib.smi_gemm_tn(epi_sel, x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), m, n, k, ldo, _stream()))
            torch.cuda.synchronize()
            outs.append(out)
    for o in outs[1:]:
        assert torch.equal(_bits(o), _bits(outs[0])), (tag, "launches differ")
    if cfg.out_tm:
        return from_tile_major(outs[0], m, no)
    assert torch.isnan(outs[0][:, no:]).all(), (tag, "wrote into the gap between rows")
    return outs[0][:, :no]


def _old(ops, epi):
    return None if epi not in R.RMW else ops.old16 if R.out_is_f16(epi) else ops.old32


def _check_dyadic(ops, epi, bias, got, tag):
    """(a): rows in blocks against the fp64 reference; returns the largest error / bound (0 for the exact epilogues)"""
    worst, old = 0.0, _old(ops, epi)
    for r0 in range(0, ops.m, BLOCK):
        r1 = min(r0 + BLOCK, ops.m)
        pre = R.preactivation(ops.x[r0:r1], ops.w, bias)
        if epi in R.LINEAR:
            want = R.round_once(R.epilogue_ref(epi, pre, None if old is None else old[r0:r1]), R.out_is_f16(epi))
            R.check_exact(got[r0:r1], want, f"{tag} rows {r0}..")
        else:
            ref, bound = R.activation_ref_bound(epi, pre)
            worst = max(worst, R.check_bound(got[r0:r1], ref, bound, f"{tag} rows {r0}.."))
    return worst


@functools.lru_cache(maxsize=2)
def _dyadic(m, n, k):
    return R.dyadic_operands(m, n, k, R.seed_of(m, n, k), device="cuda")


@functools.lru_cache(maxsize=2)
def _scaled(m, n, k):
    return R.scaled_operands(m, n, k, R.seed_of(m, n, k) + 1, device="cuda")


def _run_dyadic(lib, cfg, shape, epis, no_bias=True, pad=True):
    """(a) on one engine and shape: every epilogue with a bias, without one where `no_bias`, and (row-major) once with ldo = n + 64"""
    ops = _dyadic(*shape)
    worst = 0.0
    for epi in epis:
        variants = [(ops.bias, 0)] + ([(None, 0)] if no_bias else []) + ([(ops.bias, 64)] if pad and not cfg.out_tm else [])
        for bias, p in variants:
            got = _gemm(lib, cfg, epi, ops, bias, _old(ops, epi), pad=p)
            worst = max(worst, _check_dyadic(ops, epi, bias, got, (cfg.name, "dyadic", epi, shape, bias is not None, p)))
    print(f"{cfg.name} {shape} dyadic: epilogues {list(epis)} exact where linear (operand scale 2^{ops.scale}, {ops.inexact:.1%} of the fp16 "
          f"outputs rounded, {ops.ties:.1%} ties); activations: largest error / bound = {worst:.3f}")
    return worst


def _run_selector(lib, cfg, shape, epis, need_bias=False):
    """(b): both orientations, every phase; bias absent on even phases and zero on odd ones (always zero where the route needs one);
    the fp16 residual stream starts from zeros"""
    m, n, k = shape
    zeros = torch.zeros(n, device="cuda")
    launches = 0
    for mirrored in (False, True):
        for phase in range(R.selector_phases(n if mirrored else m, k)):
            ops = R.selector_operands(m, n, k, phase, mirrored, seed=R.seed_of(m, n, k), device="cuda")
            for epi in epis:
                assert epi in (R.BIAS, R.STORE32, R.RESID16)
                old = torch.zeros(m, n, device="cuda", dtype=torch.float16) if epi == R.RESID16 else None
                got = _gemm(lib, cfg, epi, ops, zeros if need_bias or phase % 2 else None, old)
                R.check_selector(got, ops, ops.want if R.out_is_f16(epi) else ops.want.float(), (cfg.name, "selector", epi, shape, phase, mirrored))
                launches += 1
    print(f"{cfg.name} {shape} selector: {launches} launches bit-equal to the selected operand elements")


def _run_scaled(lib, cfg, shape, epis, need_bias=False):
    """(d): the linear epilogues on real-valued operands with per-row / per-column scales, under elementwise_bound"""
    ops = _scaled(*shape)
    worst = 0.0
    for epi in epis:
        if epi not in R.LINEAR:
            continue
        old = _old(ops, epi)
        got = _gemm(lib, cfg, epi, ops, ops.bias, old)
        ref = R.gemm_tn_ref(epi, ops.x, ops.w, ops.bias, old)
        bound = R.elementwise_bound(ref, R.abs_sum(ops.x, ops.w, ops.bias, old), ops.k, R.out_is_f16(epi))
        worst = max(worst, R.check_bound(got, ref, bound, (cfg.name, "scaled", epi, shape)))
    print(f"{cfg.name} {shape} real-valued operands: largest error / elementwise bound = {worst:.3f}")
    return worst


ALL = tuple(range(10))
L1 = (R.BIAS, R.RESID32, R.STORE32, R.RESID32_HALF, R.GLU, R.RESID16, R.RESID16_HALF)    # tile-major operands, row-major output
L2 = (R.BIAS, R.RELU, R.SILU)                                                             # ... and tile-major fp16 output
L3 = (R.RESID16, R.RESID16_HALF)                                                          # ... tile-major residual stream
SEL_ROW = (R.BIAS, R.STORE32, R.RESID16)


def _no(epis, *drop):
    return tuple(e for e in epis if e not in drop)


# --------------------------------------------------------------------------------------------------------- the 128x128 family
def _ring(ring, in_tm=0, out_tm=0):
    return Cfg(f"ring{ring}" + ("-tm" if in_tm else "") + ("-otm" if out_tm else ""), dict(LONE=0), 1, in_tm, out_tm, dict(engine=RING, ring=ring))


@pytest.mark.parametrize("m,n,k", R.RING4_SHAPES)
def test_ring4_row_major(lib, m, n, k):
    """four-stage ring, 1 / 2 / 3 / 4 / 16 K tiles (shorter than, equal to and longer than the ring), 2 x 3 tiles; epilogue 9 too"""
    cfg = _ring(4)
    _run_dyadic(lib, cfg, (m, n, k), ALL)
    if k in (192, 1024):
        _run_selector(lib, cfg, (m, n, k), SEL_ROW)
    if k == 1024:
        _run_scaled(lib, cfg, (m, n, k), ALL)


@pytest.mark.parametrize("m,n,k", R.RING4_TM_SHAPES)
def test_ring4_tile_major(lib, m, n, k):
    for cfg, epis in ((_ring(4, 1), L1), (_ring(4, 1, 1), L2 + L3)):
        _run_dyadic(lib, cfg, (m, n, k), epis)
        _run_selector(lib, cfg, (m, n, k), tuple(e for e in epis if e in SEL_ROW))
    _run_scaled(lib, _ring(4, 1), (m, n, k), L1)


@pytest.mark.parametrize("m,n,k", R.RING0_SHAPES)
def test_ring0_more_tiles_than_cus(lib, m, n, k):
    """17 x 16 tiles: two stages, two workgroups per CU"""
    _run_dyadic(lib, _ring(0), (m, n, k), ALL, no_bias=False, pad=False)
    _run_dyadic(lib, _ring(0), (m, n, k), (R.BIAS, R.RESID16_HALF), no_bias=True, pad=True)
    _run_selector(lib, _ring(0), (m, n, k), SEL_ROW)
    _run_scaled(lib, _ring(0), (m, n, k), (R.BIAS, R.STORE32, R.RESID16))


def _lone64(grid, in_tm=0, out_tm=0):
    # the GLU epilogue pairs two 32-column blocks of a wave: 128-column tiles, the ring
    return Cfg("lone64" + ("-tm" if in_tm else "") + ("-otm" if out_tm else ""), dict(LONE=1, LONE16=0), 1, in_tm, out_tm,
               lambda epi: dict(engine=RING) if epi == R.GLU else dict(engine=LONE64, unit=64, grid_x=grid))


@pytest.mark.parametrize("m,n,k", R.LONE64_SHAPES)
def test_lone64_row_major(lib, m, n, k):
    """64x64 lone units: 24 units (a CU each) and 512 units (two per CU)"""
    cfg = _lone64((m // 64) * (n // 64))
    big = m * n > 1 << 20
    _run_dyadic(lib, cfg, (m, n, k), _no(ALL, R.GLU), no_bias=not big)
    _run_selector(lib, cfg, (m, n, k), SEL_ROW)
    if k == 320 or big:
        _run_scaled(lib, cfg, (m, n, k), _no(ALL, R.GLU))


@pytest.mark.parametrize("m,n,k", R.LONE64_TM_SHAPES)
def test_lone64_tile_major(lib, m, n, k):
    grid = (m // 64) * (n // 64)
    for cfg, epis in ((_lone64(grid, 1), _no(L1, R.GLU)), (_lone64(grid, 1, 1), L2 + L3)):
        _run_dyadic(lib, cfg, (m, n, k), epis)
        _run_selector(lib, cfg, (m, n, k), tuple(e for e in epis if e in SEL_ROW))


@pytest.mark.parametrize("m,n,k", R.LONE16_SHAPES)
def test_lone16(lib, m, n, k):
    """k-sliced 64x64 units: tile-major operands, K per unit 256 / 512 / 1024 (unit = 2 / 4 / 8 blocks of 128), epilogues 0, 1, 3"""
    expect = dict(engine=LONE16, unit=k // 128)
    row = Cfg("lone16-tm", dict(LONE=1, LONE16=1), 1, 1, 0, expect)
    tm = Cfg("lone16-otm", dict(LONE=1, LONE16=1), 1, 1, 1, expect)
    _run_dyadic(lib, row, (m, n, k), (R.BIAS, R.STORE32))
    _run_dyadic(lib, tm, (m, n, k), (R.BIAS, R.RELU))
    _run_selector(lib, row, (m, n, k), (R.BIAS, R.STORE32))
    _run_selector(lib, tm, (m, n, k), (R.BIAS,))
    _run_scaled(lib, row, (m, n, k), (R.BIAS, R.STORE32))
    _run_scaled(lib, tm, (m, n, k), (R.BIAS, R.RELU))


# ------------------------------------------------------------------------------------------------------- the 8-wave 256x256 engine
def _pp256(in_tm=0, out_tm=0, **more):
    layout = 0 if not in_tm else 1 if not out_tm else None
    expect = dict(engine=PP256, **more)
    return Cfg("pp256" + ("-tm" if in_tm else "") + ("-otm" if out_tm else ""), dict(G2V2=0, DEC_M160=0), 2, in_tm, out_tm,
               lambda epi: dict(expect, layout=layout if layout is not None else 3 if epi in L3 else 2))


@pytest.mark.parametrize("m,n,k", R.PP256_SHAPES)
def test_pp256(lib, m, n, k):
    """K = 64 (two slices: shorter than the pipeline lead), 192, 1024; all four layouts"""
    for cfg, epis in ((_pp256(), ALL), (_pp256(1), L1), (_pp256(1, 1), L2 + L3)):
        _run_dyadic(lib, cfg, (m, n, k), epis)
        _run_selector(lib, cfg, (m, n, k), tuple(e for e in epis if e in SEL_ROW))
    if k == 1024:
        _run_scaled(lib, _pp256(), (m, n, k), ALL)
        _run_scaled(lib, _pp256(1, 1), (m, n, k), L2 + L3)


def test_pp256_more_tiles_than_cus(lib):
    """17 x 16 tiles on 256 persistent workgroups: some walk two tiles"""
    shape = R.PP256_BIG
    _run_dyadic(lib, _pp256(grid_x=256), shape, (R.BIAS, R.STORE32, R.RESID16_HALF), no_bias=False, pad=False)
    _run_dyadic(lib, _pp256(grid_x=256), shape, (R.GLU,), no_bias=True, pad=True)
    _run_dyadic(lib, _pp256(1, 1, grid_x=256), shape, (R.RELU, R.RESID16), no_bias=False)
    _run_selector(lib, _pp256(1, 1, grid_x=256), shape, (R.BIAS, R.RESID16))


# ------------------------------------------------------------------------------------------------------- the 4-wave 256x256 engine
V2_TUNING = dict(G2V2=1, G2V2_MIN=1, DEC_M160=0)


def _v2(**more):
    return Cfg("v2", V2_TUNING, 2, 1, 1, lambda epi: dict(engine=V2_RESID if epi in L3 else V2, flag=0, layout=3 if epi in L3 else 2, **more))


@pytest.mark.parametrize("m,n,k", R.V2_SHAPES)
def test_v2(lib, m, n, k):
    """8, 12 and 32 slices; bias / relu / silu / GLU need a bias on this engine, the residual stream runs without one too"""
    cfg = _v2()
    _run_dyadic(lib, cfg, (m, n, k), L2 + (R.GLU,), no_bias=False)
    _run_dyadic(lib, cfg, (m, n, k), L3, no_bias=True)
    _run_selector(lib, cfg, (m, n, k), (R.BIAS, R.RESID16), need_bias=True)
    if k == 1024:
        _run_scaled(lib, cfg, (m, n, k), L2 + L3)


def test_v2_streams_across_tiles(lib):
    """260 tiles on 256 workgroups: four of them stream from one tile into the next"""
    cfg = _v2(grid_x=256, raster=0)
    _run_dyadic(lib, cfg, R.V2_STREAM, (R.BIAS, R.RESID16), no_bias=False)
    _run_dyadic(lib, cfg, R.V2_STREAM, (R.RESID16_HALF,), no_bias=True)
    _run_selector(lib, cfg, R.V2_STREAM, (R.BIAS, R.RESID16), need_bias=True)


def test_v2_xcd_raster(lib):
    """57 x 16 tiles under the XCD-owned raster: the last m-group has one row tile, its owner skips seven of every eight slots"""
    from sonar_amd import _lib

    with _lib.tuning(**V2_TUNING):
        info = _route(lib, R.RELU | (2 << 8) | _lib.SMI_GEMM_IN_TM | _lib.SMI_GEMM_OUT_TM, *R.V2_RASTER, R.V2_RASTER[1], True)
    assert info.raster != 0 and info.engine == V2
    _run_dyadic(lib, _v2(grid_x=256, raster=info.raster), R.V2_RASTER, (R.RELU, R.RESID16), no_bias=False)


@pytest.mark.parametrize("engine", ["ring4", "lone64", "pp256", "v2"])
def test_long_k(lib, engine):
    """K = 8192 on every engine that takes it unsplit: one dropped or doubled K element is ~0.03 on outputs of ~30, under the max-norm
    tolerance of tests/test_gpu_kernels.py and a mismatch here; the selector reads each of the 8192 positions once per orientation"""
    row = (R.BIAS, R.STORE32, R.RESID16_HALF)
    cfg, epis = {"ring4": (_ring(4), row), "lone64": (_lone64(16), row), "pp256": (_pp256(), row), "v2": (_v2(), (R.BIAS, R.RESID16_HALF))}[engine]
    _run_dyadic(lib, cfg, R.LONG_K, epis, no_bias=False, pad=False)
    _run_selector(lib, cfg, R.LONG_K, (R.BIAS,), need_bias=engine == "v2")


LONE_ENGINE = {128: V2_LONE128, 160: V2_LONE160, 192: V2_LONE192}
LONE_ROWS = {512: 128, 1280: 160, 1536: 192}


@pytest.mark.parametrize("m,n,k", R.V2_LONE_SHAPES)
def test_v2_lone_units(lib, m, n, k):
    """the 128 / 160 / 192-row lone units, tile-major out: 8, 10, 14 (and 32) slices per unit -- not multiples of the 4-slot ring,
    10 a multiple and 14 no multiple of the 192-row unit's 5 slots"""
    rows = LONE_ROWS[m]
    cfg = Cfg(f"v2_lone{rows}", dict(DEC_M160=2), 0, 1, 1, dict(engine=LONE_ENGINE[rows], unit=rows, flag=0, grid_x=(m // rows) * (n // 256)))
    _run_dyadic(lib, cfg, (m, n, k), (R.BIAS, R.RELU), no_bias=(k != 256))
    _run_selector(lib, cfg, (m, n, k), (R.BIAS,))
    if k == 448:
        _run_scaled(lib, cfg, (m, n, k), (R.BIAS, R.RELU))


# ---------------------------------------------------------------------------------------------------------------------- split-K
@functools.lru_cache(maxsize=2)
def _integer(m, n, k):
    return R.integer_operands(m, n, k, R.seed_of(m, n, k), device="cuda")


def _splitk(lib, name, tuning, expect, m, n, k, ks, in_tm, parts_of):
    """(c): fp32 and fp16 slabs, with and without a bias: slabs finite, each equal to its K range's exact sum, their sum exact"""
    from sonar_amd import _lib

    ops = _integer(m, n, k)
    x, w = _tm(ops) if in_tm else (ops.x, ops.w)
    for slab_f16, bias in ((False, ops.bias), (True, ops.bias), (True, None)):
        tag = (name, (m, n, k, ks), "fp16 slabs" if slab_f16 else "fp32 slabs", bias is not None)
        want = expect(slab_f16) if callable(expect) else expect
        if want is None:
            continue
        runs = []
        with _lib.tuning(**tuning):
            info = _route(lib, _lib.SMI_GEMM_IN_TM if in_tm else 0, m, n, k, n, bias is not None, ksplit=ks, slab_f16=slab_f16)
            _assert_route(info, dict(want, ksplit=ks, part_stride=m * n * (2 if slab_f16 else 4)), tag)
            for _ in range(2):
                parts = _nan((ks, m, n), torch.float16 if slab_f16 else torch.float32)
                _lib.check(lib.smi_gemm_tn_splitk(x.data_ptr(), w.data_ptr(), _ptr(bias), parts.data_ptr(), m, n, k, ks, in_tm,
                                                  _lib.SMI_F16 if slab_f16 else _lib.SMI_F32, _stream()))
                torch.cuda.synchronize()
                runs.append(parts)
        assert torch.equal(_bits(runs[0]), _bits(runs[1])), (tag, "launches differ")
        assert torch.isfinite(runs[0]).all(), tag
        total = R.preactivation(ops.x, ops.w, bias)
        R.check_exact(runs[0].double().sum(0), total, f"{tag} sum of the slabs")
        slabs = R.splitk_ref(ops.x, ops.w, bias, parts_of(k, ks))
        for z in range(ks):
            R.check_exact(runs[0][z].double(), slabs[z], f"{tag} slab {z}")
    print(f"{name} split-K {(m, n, k, ks)}: fp32 and fp16 slabs and their sums exact")


@pytest.mark.parametrize("m,n,k,ks", R.SPLITK_SMALL)
def test_splitk_ring_and_lone64(lib, m, n, k, ks):
    _splitk(lib, "ring4", dict(LONE=0), dict(engine=RING, ring=4, grid_y=ks), m, n, k, ks, 0, R.even_parts)
    _splitk(lib, "lone64", dict(LONE=1, LONE16=0), dict(engine=LONE64, grid_y=ks), m, n, k, ks, 0, R.even_parts)


@pytest.mark.parametrize("m,n,k,ks", R.SPLITK_LONE16)
def test_splitk_lone16(lib, m, n, k, ks):
    _splitk(lib, "lone16", dict(LONE=1, LONE16=1, DEC_M160=0), dict(engine=LONE16, unit=k // ks // 128, grid_y=ks), m, n, k, ks, 1, R.even_parts)


@pytest.mark.parametrize("m,n,k,ks", R.SPLITK_PP256)
def test_splitk_pp256(lib, m, n, k, ks):
    """the 8-wave engine's split-K: 50 slices in 3 parts (16, 17, 17 slices) and an even split, row-major and tile-major operands"""
    for in_tm in (0, 1):
        _splitk(lib, "pp256" + ("-tm" if in_tm else ""), dict(G2_SPLITK_MIN=1, DEC_M160=0), dict(engine=PP256, layout=in_tm), m, n, k, ks,
                in_tm, R.slice_parts)


@pytest.mark.parametrize("m,n,k,ks", R.V2_LONE_SLAB_SHAPES)
def test_splitk_v2_lone_units(lib, m, n, k, ks):
    """fp16 slabs of the lone units (fp32 slabs of the same request go elsewhere: not asserted here), 10 and 14 slices per unit"""
    rows = LONE_ROWS[m]
    want = dict(engine=LONE_ENGINE[rows], unit=rows, flag=1, grid_x=(m // rows) * (n // 256) * ks)
    _splitk(lib, f"v2_lone{rows}", dict(DEC_M160=2), lambda slab_f16: want if slab_f16 else None, m, n, k, ks, 1, R.even_parts)


# -------------------------------------------------------------------------------------------- logits with tile statistics
def _stats_logits(lib, engine, ops, valid_n, scale=0.125):
    from sonar_amd import _lib

    m, n, k = ops.m, ops.n, ops.k
    x, w = _tm(ops)
    tuning = dict(G2V2=1, G2V2_MIN=1) if engine == V2_STATS else dict(G2V2=0)
    runs = []
    with _lib.tuning(**tuning):
        info = _route(lib, _lib.SMI_GEMM_IN_TM | _lib.SMI_GEMM_OUT_TM, m, n, k, n, False, stats=1)
        _assert_route(info, dict(engine=engine, layout=2), ("tile stats", engine, (m, n, k)))
        for _ in range(2):
            out, tmax, tsum = _nan((m * n,), torch.float16), _nan((n // 256, m), torch.float32), _nan((n // 256, m), torch.float32)
            _lib.check(lib.smi_gemm_tn_tile_stats(x.data_ptr(), w.data_ptr(), out.data_ptr(), m, n, k, scale, valid_n, tmax.data_ptr(),
                                                  tsum.data_ptr(), _stream()))
            torch.cuda.synchronize()
            runs.append((out, tmax, tsum))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs)), "launches differ"
    assert torch.isfinite(runs[0][1]).all() and torch.isfinite(runs[0][2]).all()
    return from_tile_major(runs[0][0], m, n)


@pytest.mark.parametrize("engine", [V2_STATS, PP256])
@pytest.mark.parametrize("m,n,k,valid_n", R.STATS_SHAPES)
def test_tile_stats_logits(lib, m, n, k, valid_n, engine):
    """the logits of the fused statistics passes (the statistics stay with tests/test_gpu_kernels.py): all n columns stored, the
    masked last tile included"""
    ops = _dyadic(m, n, k)
    R.check_exact(_stats_logits(lib, engine, ops, valid_n), R.round_once(R.preactivation(ops.x, ops.w), True), ("stats dyadic", engine))
    for mirrored in (False, True):
        for phase in range(R.selector_phases(n if mirrored else m, k)):
            sel = R.selector_operands(m, n, k, phase, mirrored, seed=5, device="cuda")
            R.check_selector(_stats_logits(lib, engine, sel, valid_n), sel, tag=("stats selector", engine, phase, mirrored))
    sc = _scaled(m, n, k)
    ref = R.preactivation(sc.x, sc.w)
    worst = R.check_bound(_stats_logits(lib, engine, sc, valid_n), ref, R.elementwise_bound(ref, R.abs_sum(sc.x, sc.w), k, True), "stats scaled")
    print(f"tile-stats logits engine {engine} {(m, n, k)} valid_n {valid_n}: dyadic and selector exact; largest error / elementwise bound = {worst:.3f}")


def test_every_engine_was_asserted():
    """runs last: the cases above pinned and asserted each of the ten engines at least once.  Only meaningful when the whole file
    runs in one process: under -k, --lf or a single-test run it fails for the engines whose cases were not selected."""
    from sonar_amd import _lib

    missing = [_lib.GEMM_ENGINE_NAMES[e] for e in range(1, len(_lib.GEMM_ENGINE_NAMES)) if e not in ROUTED]
    assert not missing, missing
