"""GPU: the beam search's state kernels -- vocab_select, beam_init, beam_step, beam_reorder, beam_output -- driven position by
position from Python on synthetic logits and compared after every launch with the restatement of tests/beam_ref.py.

Integers (tokens, parents, counters, histories, ancestry, finished hypotheses) are compared exactly; pval and pmax bit for bit.
The floats new_cum / fin_score / margins are held to the error model of beam_ref (B_STEP, derived from the kernel's fp32 expression
(cum + v) - (pmax + __logf(psum))); to keep rounding from compounding the reference's step takes the device's own fp32 cum.  The
inputs satisfy the gap condition (tests/test_beam_ref_cpu.py asserts it for every case): neighbours inside a decision range are tied
by construction or 16 B apart, so no case is excused or skipped.  Every output array, and every input row that must not be read
(rows at or beyond nactive, rows of finished sentences, the lists after a k2 = 0 launch), is poisoned first.

Measured on an MI355X (profiles/beam_kernels_pytest_gpu.log):
  L, the error of pmax + __logf(psum) against the float64 log-sum-exp on the first free step of every case (it includes the three
  fp32 roundings of the step's expression at that step's magnitudes): worst 9.8e-7 -> beam_ref.L_LOG = 4e-6 (4 x, rounded up);
  the relative error of fin_score's raw / __powf(step, len_penalty) against float64 (len_penalty 0.5, 1 and 2, steps 1 to 8; the
  division's rounding included): worst 7.1e-8 -> POW_REL = 3e-7 (4 x, rounded up).
Both are hardware intrinsics: the factor 4 covers arguments the tests do not sample."""
import ctypes as C
import math

import pytest
import torch

from tests import beam_ref as R

pytestmark = pytest.mark.gpu

INT_MAX = 0x7FFFFFFF
SENT = -77            # sentinel of the integer arrays
POW_REL = 3e-7        # see the module docstring
MEASURED = {"L": 0.0}


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib

    handle = _lib.load()
    _lib.check(handle.smi_init(0))
    return handle


def _to_tile_major(a):
    """tile-major layout of include/sonar_mi355.h (as tests/test_gpu_kernels.py states it)."""
    rows, k = a.shape
    rr = torch.arange(256, device=a.device)
    q = (rr >> 2) & 3
    swz = q ^ ((q & 1) << 1)
    blocks = a.view(rows // 256, 256, k // 32, 4, 8).permute(0, 2, 1, 3, 4)
    slot = torch.arange(4, device=a.device)
    idx = (slot[None, :] ^ swz[:, None])[None, None, :, :, None].expand(rows // 256, k // 32, 256, 4, 8)
    return torch.gather(blocks, 3, idx).contiguous().view(-1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ints(shape, fill=SENT):
    shape = shape if isinstance(shape, tuple) else (shape,)
    return torch.full(shape, fill, dtype=torch.int32, device="cuda")


def _nans(shape):
    shape = shape if isinstance(shape, tuple) else (shape,)
    return torch.full(shape, math.nan, dtype=torch.float32, device="cuda")


def _table_struct(_lib, tab):
    if tab is None:
        return _lib.smi_prompt_table()
    return _lib.smi_prompt_table(tok=tab["tok"].data_ptr(), len=tab["len"].data_ptr(), stride=tab["stride"], gen_cap=tab["gen_cap"],
                                 min_gen=tab["min_gen"], model_max=tab["model_max"])


def _upload_logits(scaled_raw, vocab, f16_tm):
    """scaled_raw: CPU fp32 [rows, vocab] raw logits (NaN rows = must not be read).  -> device logits in the asked format (columns
    >= vocab and padding rows NaN) and ldl."""
    rows = scaled_raw.shape[0]
    ldl = (vocab + 255) // 256 * 256
    full = torch.full(((rows + 255) // 256 * 256 if f16_tm else rows, ldl), math.nan, dtype=torch.float32)
    full[:rows, :vocab] = scaled_raw
    full = full.cuda()
    return (_to_tile_major(full.half()) if f16_tm else full.contiguous()), ldl


def _tile_stats(scaled, vocab):
    """as the logits GEMM's epilogue leaves them: per 256-column tile of the SCALED logits, maximum and sum of exp(v - maximum)"""
    rows = scaled.shape[0]
    ldl = (vocab + 255) // 256 * 256
    lg = torch.full((rows, ldl), -math.inf, dtype=torch.float32)
    lg[:, :vocab] = scaled
    t = lg.view(rows, ldl // 256, 256)
    tmax = t.max(dim=2).values
    tsum = torch.where(torch.isinf(t) & (t < 0), torch.zeros_like(t), torch.exp(t - tmax[:, :, None])).sum(dim=2)
    tsum = torch.where(torch.isinf(tmax), torch.zeros_like(tsum), tsum)
    return tmax.t().contiguous().cuda(), tsum.t().contiguous().cuda()


def _select(lib, logits_dev, ldl, f16_tm, rows, vocab, tile_max, tile_sum, k2, inv_temp, pad, eos, unk, unk_penalty, block_eos,
            out, tab=None, group=1, step_nr=1):
    from sonar_amd import _lib

    a = _lib.smi_vocab_select_args(
        logits=logits_dev.data_ptr(), ldl=ldl, logits_f16_tm=1 if f16_tm else 0, rows=rows, vocab=vocab, tile_max=tile_max.data_ptr(),
        tile_sum=tile_sum.data_ptr(), stat_rows=tile_max.shape[1], k2=k2, inv_temp=inv_temp, pad_idx=pad, eos_idx=eos, unk_idx=unk,
        unk_penalty=unk_penalty, block_eos=1 if block_eos else 0, pmax=out["pmax"].data_ptr(), psum=out["psum"].data_ptr(),
        pval=out["pval"].data_ptr(), pidx=out["pidx"].data_ptr(), table=_table_struct(_lib, tab), group=group, step_nr=step_nr)
    _lib.check(lib.smi_vocab_select(C.byref(a), _stream()))
    torch.cuda.synchronize()


def _expected_list(scaled_row, k2, pad, eos, unk, unk_penalty, block_eos):
    """fp32, the kernel's own arithmetic: (value bits, tokens) of the masked row's best k2, value desc, token asc"""
    v = scaled_row.clone()
    if unk >= 0:
        v[unk] = v[unk] - torch.tensor(unk_penalty, dtype=torch.float32)
    if pad >= 0:
        v[pad] = -math.inf
    if block_eos and eos >= 0:
        v[eos] = -math.inf
    sv, si = torch.sort(v, descending=True, stable=True)
    sv, si = sv[:k2].clone(), si[:k2].to(torch.int32)
    si[torch.isinf(sv)] = INT_MAX
    return sv, si


# ----------------------------------------------------------------------------------------------------------- the driver
class Search:
    """One search on the device, launch by launch, with its arrays on the host side for the comparisons."""

    def __init__(self, lib, case, f16_tm):
        from sonar_amd import _lib

        self.lib, self._lib, self.case, self.f16_tm = lib, _lib, case, f16_tm
        P, plans = case.P, case.plans
        self.n, self.beam, self.rows = len(plans), P.beam, len(plans) * P.beam
        self.vocab = case.logits.vocab
        self.maxlen_hi = max(p.max_len for p in plans)
        self.stride = self.maxlen_hi + 1
        n, rows, st = self.n, self.rows, self.stride
        self.a = dict(tok=_ints(rows), cum=_nans(rows), nactive=_ints(n), done=_ints(n), ndone=_ints(1), parent=_ints(rows),
                      new_tok=_ints(rows), new_cum=_nans(rows), fin_tok=_ints((rows, st)), fin_len=_ints(rows), fin_score=_nans(rows),
                      fin_count=_ints(n), margins=_nans((n, 2)), anc=_ints((2, rows, st)), hist=_ints((2, rows, st)))
        self.sel = dict(pmax=_nans(rows), psum=_nans(rows), pval=_nans((rows, 16)), pidx=_ints((rows, 16)))
        self.state = _lib.smi_beam_state(**{k: self.a[k].data_ptr() for k in ("tok", "cum", "nactive", "done", "ndone", "parent", "new_tok",
                                                                             "new_cum", "fin_tok", "fin_len", "fin_score", "fin_count",
                                                                             "margins")}, n=n, beam=self.beam, stride=st)
        for i in range(2):
            self.state.anc[i] = self.a["anc"][i].data_ptr()
            self.state.hist[i] = self.a["hist"][i].data_ptr()
        self.tab = None
        if case.table:
            width = max(p.plen for p in plans)
            tok = torch.full((n, width), SENT, dtype=torch.int32)
            for s, p in enumerate(plans):
                tok[s, :p.plen] = torch.tensor(p.prompt, dtype=torch.int32)
            self.tab = dict(tok=tok.cuda(), len=torch.tensor([p.plen for p in plans], dtype=torch.int32).cuda(), stride=width,
                            gen_cap=plans[0].gen_cap, min_gen=plans[0].min_gen, model_max=plans[0].model_max)
        self.inv_temp = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(P.temperature, dtype=torch.float32))
        self.trace = []       # every array after every launch: two runs must agree bit for bit
        self.first_free_seen = False

    def host(self):
        torch.cuda.synchronize()
        h = {k: v.cpu() for k, v in self.a.items()}
        self.trace.append({k: _bits(v).clone() for k, v in h.items()})
        return h

    # ---- what generate_chain's host schedule does at the step that chooses token step_nr
    def schedule(self, step_nr):
        plans = self.case.plans
        pmin, pmax = min(p.plen for p in plans), max(p.plen for p in plans)
        lo, hi = min(p.max_len for p in plans), max(p.max_len for p in plans)
        mlo, mhi = min(p.min_len for p in plans), max(p.min_len for p in plans)
        if step_nr < pmin:
            kind = "forced"
        elif step_nr >= pmax and lo == hi and step_nr == lo - 1:
            kind = "eos"
        elif step_nr >= pmax and step_nr < lo - 1 and step_nr < mlo:
            kind = "free_blocked"
        elif step_nr >= pmax and step_nr < lo - 1 and step_nr >= mhi:
            kind = "free"
        else:
            kind = "mixed"
        step_table = self.tab is not None and not (pmin == pmax and step_nr >= pmax)
        return kind, step_table, pmax, hi

    def init(self):
        plans = self.case.plans
        if self.tab is None:
            rc = self.lib.smi_beam_init(C.byref(self.state), plans[0].prompt[0], None, 0, _stream())
        else:
            rc = self.lib.smi_beam_init(C.byref(self.state), 0, self.tab["tok"].data_ptr(), self.tab["stride"], _stream())
        self._lib.check(rc)
        h = self.host()
        first = torch.tensor([p.prompt[0] for p in plans], dtype=torch.int32).repeat_interleave(self.beam)
        assert torch.equal(h["tok"], first) and torch.equal(_bits(h["cum"]), torch.zeros(self.rows, dtype=torch.int32))
        assert torch.equal(h["nactive"], torch.ones(self.n, dtype=torch.int32))
        assert not h["done"].any() and not h["fin_count"].any() and h["ndone"].item() == 0
        assert torch.isinf(h["margins"]).all() and (h["margins"] > 0).all()
        want = torch.full((2, self.rows, self.stride), SENT, dtype=torch.int32)
        want[0, :, 0] = first
        assert torch.equal(h["hist"], want)
        want[0, :, 0] = torch.arange(self.rows, dtype=torch.int32)
        assert torch.equal(h["anc"], want)
        for k in ("parent", "new_tok", "fin_tok", "fin_len"):
            assert (h[k] == SENT).all(), k
        assert torch.isnan(h["new_cum"]).all() and torch.isnan(h["fin_score"]).all()
        return h

    def step(self, pos, h, check=True):
        """selection + beam step + reorder at position pos; h: the host copy of the state before it.  -> the state after."""
        P, plans, beam, n, vocab = self.case.P, self.case.plans, self.beam, self.n, self.vocab
        step_nr, cur = pos + 1, pos & 1
        kind, step_table, pmax_len, maxlen_hi = self.schedule(step_nr)
        # ---- logits of the live rows; every other row is NaN: it must not be read by the beam step
        raw = torch.full((self.rows, vocab), math.nan, dtype=torch.float32)
        live = []
        for s in range(n):
            if h["done"][s]:
                continue
            for r in range(int(h["nactive"][s])):
                row = s * beam + r
                raw[row] = self.case.logits(s, h["hist"][cur, row, :pos + 1].tolist())
                live.append(row)
        scaled = raw * torch.tensor(self.inv_temp, dtype=torch.float32)
        dev_logits, ldl = _upload_logits(raw, vocab, self.f16_tm)
        tile_max, tile_sum = _tile_stats(scaled, vocab)
        # ---- the selection, as generate_chain asks for it
        free = kind in ("free", "free_blocked", "mixed")
        for k in ("pmax", "psum", "pval"):
            self.sel[k].fill_(math.nan)
        self.sel["pidx"].fill_(SENT)
        _select(self.lib, dev_logits, ldl, self.f16_tm, self.rows, vocab, tile_max, tile_sum, 2 * beam if free else 0, self.inv_temp,
                P.pad_idx, P.eos_idx, P.unk_idx, P.unk_penalty if free else 0.0, kind == "free_blocked", self.sel,
                tab=self.tab if kind == "mixed" else None, group=beam, step_nr=step_nr)
        sel = {k: v.cpu() for k, v in self.sel.items()}
        self.trace.append({k: _bits(v).clone() for k, v in sel.items()})
        if check:
            for row in live:
                s = row // beam
                mode = plans[s].mode(step_nr)
                assert _same_bits(sel["pmax"][row], scaled[row].max()), (pos, row)
                true_sum = torch.exp(scaled[row].double() - scaled[row].max().double()).sum().item()
                assert abs(sel["psum"][row].item() - true_sum) <= 0.5 * R.L_LOG * true_sum, (pos, row)
                if mode == "free":
                    ev, ei = _expected_list(scaled[row], 2 * beam, P.pad_idx, P.eos_idx, P.unk_idx, P.unk_penalty, step_nr < plans[s].min_len)
                    assert torch.equal(sel["pidx"][row, :2 * beam], ei) and _same_bits(sel["pval"][row, :2 * beam], ev), (pos, row)
                    assert (sel["pidx"][row, 2 * beam:] == SENT).all() and torch.isnan(sel["pval"][row, 2 * beam:]).all()
                else:   # a forced row, by k2 = 0 or by the table exit: the normaliser only
                    assert (sel["pidx"][row] == SENT).all() and torch.isnan(sel["pval"][row]).all(), (pos, row)
        # rows the beam step must not read: their lists and normalisers are poisoned whatever the selection left there
        dead = torch.ones(self.rows, dtype=torch.bool)
        dead[live] = False
        dead = dead.cuda()
        for k in ("pmax", "psum", "pval"):
            self.sel[k][dead] = math.nan
        self.sel["pidx"][dead] = SENT
        # ---- the beam step
        self.a["parent"].fill_(SENT)
        self.a["new_tok"].fill_(SENT)
        self.a["new_cum"].fill_(math.nan)
        b = self._lib.smi_beam_step_args(
            logits=dev_logits.data_ptr(), ldl=ldl, logits_f16_tm=1 if self.f16_tm else 0, vocab=vocab, pmax=self.sel["pmax"].data_ptr(),
            psum=self.sel["psum"].data_ptr(), pval=self.sel["pval"].data_ptr(), pidx=self.sel["pidx"].data_ptr(), k2=2 * beam, pos=pos,
            prompt_len=pmax_len if not step_table else 1, forced_tok=plans[0].prompt[step_nr] if self.tab is None and kind == "forced" else -1,
            max_len=maxlen_hi, inv_temp=self.inv_temp, len_penalty=P.len_penalty, normalize=1 if P.normalize else 0, eos_idx=P.eos_idx,
            table=_table_struct(self._lib, self.tab if step_table else None))
        self._lib.check(self.lib.smi_beam_step(C.byref(self.state), C.byref(b), _stream()))
        g = self.host()
        if check:
            self.check_step(pos, h, g, raw, scaled, sel)
        # ---- the reorder
        self._lib.check(self.lib.smi_beam_reorder(C.byref(self.state), pos, _stream()))
        a = self.host()
        if check:
            self.check_reorder(pos, g, a)
        return a

    def check_step(self, pos, h, g, raw, scaled, sel):
        P, plans, beam, n = self.case.P, self.case.plans, self.beam, self.n
        step_nr, cur = pos + 1, pos & 1
        B = R.B_STEP
        want = {k: h[k].clone() for k in ("nactive", "done", "fin_tok", "fin_len", "fin_count")}
        ident = torch.arange(self.rows, dtype=torch.int32)
        for s in range(n):
            base = s * beam
            sl = slice(base, base + beam)
            if h["done"][s]:   # inert, bit for bit
                assert torch.equal(g["parent"][sl], ident[sl]) and torch.equal(g["new_tok"][sl], h["tok"][sl]), (pos, s)
                assert _same_bits(g["new_cum"][sl], h["cum"][sl]) and _same_bits(g["margins"][s], h["margins"][s]), (pos, s)
                assert _same_bits(g["fin_score"][sl], h["fin_score"][sl]), (pos, s)
                continue
            na, nfin = int(h["nactive"][s]), int(h["fin_count"][s])
            rows = [R.Row(h["hist"][cur, base + r, :pos + 1].tolist(), float(h["cum"][base + r])) for r in range(na)]
            o = R.step(P, plans[s], step_nr, rows, raw[base:base + na], nfin)
            assert max(abs(r.cum) for r in rows) <= R.CUM_MAX
            if o.kind == "free" and not self.first_free_seen:
                # L: pmax + __logf(psum) against the float64 log-sum-exp, through the step's own expression
                for w, (_, _, c) in enumerate(o.cont):
                    MEASURED["L"] = max(MEASURED["L"], abs(g["new_cum"][base + w].item() - c))
            # finished hypotheses
            for f, (r, raw_score, score, _) in enumerate(o.fin):
                slot = base + nfin + f
                toks = rows[r].hist[plans[s].plen:] + [P.eos_idx]
                want["fin_tok"][slot, :len(toks)] = torch.tensor(toks, dtype=torch.int32)
                want["fin_len"][slot] = len(toks)
                tol = B / float(step_nr) ** P.len_penalty if P.normalize else B
                tol += (POW_REL + 2.0 ** -23) * abs(score) if P.normalize else 0.0
                assert abs(g["fin_score"][slot].item() - score) <= tol, (pos, s, f, g["fin_score"][slot].item(), score, tol)
            want["fin_count"][s] = nfin + len(o.fin)
            untouched = [i for i in range(beam) if not nfin <= i < nfin + len(o.fin)]
            assert _same_bits(g["fin_score"][base:base + beam][untouched], h["fin_score"][base:base + beam][untouched]), (pos, s)
            if o.done:
                want["done"][s] = 1
            if o.done or not o.cont:
                assert torch.equal(g["parent"][sl], ident[sl]) and torch.equal(g["new_tok"][sl], h["tok"][sl]), (pos, s)
                assert _same_bits(g["new_cum"][sl], h["cum"][sl]), (pos, s)
            else:
                w = len(o.cont)
                assert g["parent"][base:base + w].tolist() == [base + p for p, _, _ in o.cont], (pos, s, g["parent"][sl].tolist(), o.cont)
                assert g["new_tok"][base:base + w].tolist() == [t for _, t, _ in o.cont], (pos, s, g["new_tok"][sl].tolist(), o.cont)
                for i, (_, _, c) in enumerate(o.cont):
                    assert abs(g["new_cum"][base + i].item() - c) <= B, (pos, s, i, g["new_cum"][base + i].item(), c)
                # the spare slots: themselves, and -inf after a free step (the forced prompt step leaves their cum)
                assert torch.equal(g["parent"][base + w:base + beam], ident[base + w:base + beam]), (pos, s)
                assert torch.equal(g["new_tok"][base + w:base + beam], h["tok"][base + w:base + beam]), (pos, s)
                if o.kind == "free":
                    want["nactive"][s] = w
                    assert (g["new_cum"][base + w:base + beam] == -math.inf).all(), (pos, s)
                else:
                    assert _same_bits(g["new_cum"][base + w:base + beam], h["cum"][base + w:base + beam]), (pos, s)
            # the margin of the steps
            m_want = min(h["margins"][s, 0].item(), o.margin)
            m_got = g["margins"][s, 0].item()
            assert m_got == m_want if math.isinf(m_want) or m_want == 0.0 else abs(m_got - m_want) <= 2 * B, (pos, s, m_got, m_want)
            assert _same_bits(g["margins"][s, 1], h["margins"][s, 1])
        self.first_free_seen = self.first_free_seen or any(plans[s].mode(step_nr) == "free" and not h["done"][s] for s in range(n))
        for k, v in want.items():
            assert torch.equal(g[k], v), (pos, k)
        assert g["ndone"].item() == int(want["done"].sum())
        for k in ("tok", "cum", "anc", "hist"):   # the step writes none of these
            assert _same_bits(g[k], h[k]), (pos, k)

    def check_reorder(self, pos, g, a):
        cur = pos & 1
        par = g["parent"].long()
        want_h, want_a = g["hist"].clone(), g["anc"].clone()
        want_h[cur ^ 1, :, :pos + 1] = g["hist"][cur, par, :pos + 1]
        want_h[cur ^ 1, :, pos + 1] = g["new_tok"]
        want_a[cur ^ 1, :, :pos] = g["anc"][cur, par, :pos]
        want_a[cur ^ 1, :, pos] = g["parent"]
        assert torch.equal(a["hist"], want_h) and torch.equal(a["anc"], want_a), pos
        assert torch.equal(a["tok"], g["new_tok"]) and _same_bits(a["cum"], g["new_cum"]), pos
        for k in ("nactive", "done", "ndone", "parent", "new_tok", "new_cum", "fin_tok", "fin_len", "fin_score", "fin_count", "margins"):
            assert _same_bits(a[k], g[k]), (pos, k)

    def output(self, out_stride):
        out = dict(tok=_ints((self.rows, out_stride)), len=_ints(self.rows), score=_nans(self.rows))
        self._lib.check(self.lib.smi_beam_output(C.byref(self.state), out_stride, out["tok"].data_ptr(), out["len"].data_ptr(),
                                                 out["score"].data_ptr(), _stream()))
        torch.cuda.synchronize()
        o = {k: v.cpu() for k, v in out.items()}
        self.trace.append({k: _bits(v).clone() for k, v in o.items()})
        return o

    def run(self, check=True):
        h = self.init()
        for pos in range(self.maxlen_hi - 1):
            h = self.step(pos, h, check)
        before = self.host()
        out = self.output(self.maxlen_hi)
        after = self.host()
        return before, out, after


def _run_case(lib, name, f16_tm):
    case = R.CASES[name]
    P, plans, beam = case.P, case.plans, case.P.beam
    S = Search(lib, case, f16_tm)
    h, out, after = S.run()
    assert h["done"].all() and h["ndone"].item() == len(plans) and (h["fin_count"] == beam).all()
    for k in h:
        if k != "margins":
            assert _same_bits(h[k], after[k]), k
    assert _same_bits(h["margins"][:, 0], after["margins"][:, 0])
    # ---- the whole search against the free-running float64 reference: every hypothesis of every sentence
    ref = R.search(P, plans, case.logits)
    nsteps = S.maxlen_hi
    for s, hyps in enumerate(ref.hyps):
        for i, (toks, score) in enumerate(hyps):
            row = s * beam + i
            assert out["len"][row].item() == len(toks) and out["tok"][row, :len(toks)].tolist() == toks, (s, i, out["tok"][row].tolist(), toks)
            assert (out["tok"][row, len(toks):] == -1).all()
            tol = nsteps * R.B_STEP + (POW_REL + 2.0 ** -23) * abs(score)
            assert abs(out["score"][row].item() - score) <= tol, (s, i, out["score"][row].item(), score)
        # the returned scores are the finished ones, sorted; the final margin is best minus second
        fs = h["fin_score"][s * beam:(s + 1) * beam]
        assert _same_bits(out["score"][s * beam:(s + 1) * beam], torch.sort(fs, descending=True, stable=True).values)
        m1 = after["margins"][s, 1]
        if beam >= 2:
            assert _same_bits(m1, out["score"][s * beam] - out["score"][s * beam + 1])
            assert abs(m1.item() - ref.margins[s][1]) <= 2 * nsteps * R.B_STEP + 2 * POW_REL * abs(hyps[0][1])
        else:
            assert _same_bits(m1, h["margins"][s, 1])
        m0 = after["margins"][s, 0].item()
        assert m0 == ref.margins[s][0] if math.isinf(ref.margins[s][0]) or ref.margins[s][0] == 0.0 else abs(m0 - ref.margins[s][0]) <= 2 * nsteps * R.B_STEP
    print(f"[beam kernels] {name} f16_tm={int(f16_tm)}: L, worst over the first free steps so far {MEASURED['L']:.3e} (allowed {R.L_LOG:.1e})")
    assert MEASURED["L"] <= R.L_LOG
    return S


GENERAL = [n for n in R.CASES if n.startswith("general")]
OTHERS = [n for n in R.CASES if not n.startswith("general")]


@pytest.mark.parametrize("f16_tm", [False, True], ids=["f32", "f16tm"])
@pytest.mark.parametrize("name", GENERAL)
def test_general_search_step_by_step_and_twice(lib, name, f16_tm):
    S = _run_case(lib, name, f16_tm)
    T = Search(lib, R.CASES[name], f16_tm)
    T.run(check=False)
    assert len(S.trace) == len(T.trace)
    for i, (a, b) in enumerate(zip(S.trace, T.trace)):   # two identical runs: every array after every launch, bit for bit
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)


@pytest.mark.parametrize("f16_tm", [False, True], ids=["f32", "f16tm"])
@pytest.mark.parametrize("name", OTHERS)
def test_search_step_by_step(lib, name, f16_tm):
    _run_case(lib, name, f16_tm)


def test_fast_pow_error(lib):
    """fin_score = raw / __powf(step, len_penalty): the same search with and without normalisation has the same raw scores, bit
    for bit, so their quotient against the float64 power isolates the fast pow (and the division's one rounding)."""
    import dataclasses

    base = R.CASES["unnormalized"]
    raw_run = Search(lib, base, False).run(check=False)[0]
    worst = 0.0
    for lp in (0.5, 1.0, 2.0):
        case = dataclasses.replace(base, P=dataclasses.replace(base.P, normalize=True, len_penalty=lp))
        h = Search(lib, case, False).run(check=False)[0]
        assert torch.equal(h["fin_tok"], raw_run["fin_tok"]) and torch.equal(h["fin_len"], raw_run["fin_len"])
        steps = raw_run["fin_len"].double()   # prompts of one token: the step that finished a hypothesis is its length
        want = raw_run["fin_score"].double() / steps ** lp
        worst = max(worst, ((h["fin_score"].double() / want) - 1.0).abs().max().item())
    print(f"[beam kernels] __powf(step, len_penalty) with the division, relative to float64: worst {worst:.3e} (allowed {POW_REL:.1e})")
    assert worst <= POW_REL


# ------------------------------------------------------------------------------------------------------ reorder alone
@pytest.mark.parametrize("pos", [0, 1, 255, 256, 300])
def test_reorder_alone(lib, pos):
    from sonar_amd import _lib

    n, beam, stride = 5, 3, 304
    rows = n * beam
    g = torch.Generator().manual_seed(pos)
    # parents stay inside their sentence; duplicates (one parent, several children) and plain permutations
    parent = torch.cat([s * beam + (torch.tensor([1, 1, 0]) if s % 2 else torch.randperm(beam, generator=g)) for s in range(n)]).to(torch.int32)
    a = dict(tok=_ints(rows), cum=_nans(rows), nactive=_ints(n), done=_ints(n), ndone=_ints(1), parent=parent.cuda(),
             new_tok=torch.randint(0, 1000, (rows,), generator=g, dtype=torch.int32).cuda(),
             new_cum=torch.randn(rows, generator=g).cuda(), fin_tok=_ints((rows, stride)), fin_len=_ints(rows), fin_score=_nans(rows),
             fin_count=_ints(n), margins=_nans((n, 2)),
             anc=torch.randint(0, rows, (2, rows, stride), generator=g, dtype=torch.int32).cuda(),
             hist=torch.randint(0, 1000, (2, rows, stride), generator=g, dtype=torch.int32).cuda())
    cur = pos & 1
    a["anc"][cur ^ 1].fill_(SENT)
    a["hist"][cur ^ 1].fill_(SENT)
    st = _lib.smi_beam_state(**{k: a[k].data_ptr() for k in a if k not in ("anc", "hist")}, n=n, beam=beam, stride=stride)
    for i in range(2):
        st.anc[i], st.hist[i] = a["anc"][i].data_ptr(), a["hist"][i].data_ptr()
    before = {k: v.cpu() for k, v in a.items()}
    outs = []
    for _ in range(2):
        _lib.check(lib.smi_beam_reorder(C.byref(st), pos, _stream()))
        torch.cuda.synchronize()
        outs.append({k: v.cpu() for k, v in a.items()})
    got = outs[0]
    par = before["parent"].long()
    want_h = torch.full((rows, stride), SENT, dtype=torch.int32)
    want_a = want_h.clone()
    want_h[:, :pos + 1] = before["hist"][cur, par, :pos + 1]
    want_h[:, pos + 1] = before["new_tok"]
    want_a[:, :pos] = before["anc"][cur, par, :pos]
    want_a[:, pos] = before["parent"]
    assert torch.equal(got["hist"][cur ^ 1], want_h) and torch.equal(got["anc"][cur ^ 1], want_a)   # beyond pos + 1 (pos): the sentinels
    assert torch.equal(got["hist"][cur], before["hist"][cur]) and torch.equal(got["anc"][cur], before["anc"][cur])
    assert torch.equal(got["tok"], before["new_tok"]) and _same_bits(got["cum"], before["new_cum"])
    for k in ("nactive", "done", "ndone", "parent", "new_tok", "new_cum", "fin_tok", "fin_len", "fin_score", "fin_count", "margins"):
        assert _same_bits(got[k], before[k]), k
    for k in got:
        assert _same_bits(got[k], outs[1][k]), k


# ------------------------------------------------------------------------------------------------------- output alone
@pytest.mark.parametrize("beam", [1, 3, 8])
def test_output_alone(lib, beam):
    from sonar_amd import _lib

    n, stride, out_stride = beam + 2, 14, 9
    rows = n * beam
    g = torch.Generator().manual_seed(beam)
    fin_count = torch.tensor([min(s, beam) for s in range(n)], dtype=torch.int32)          # 0 .. beam
    fin_len = torch.randint(1, out_stride + 1, (rows,), generator=g, dtype=torch.int32)
    fin_len[-1] = out_stride                                                                # a hypothesis as long as the output row
    # scores from a set of three values: equal ones everywhere, so the order among them shows the sort is stable
    fin_score = torch.tensor([-1.5, -2.25, -0.75])[torch.randint(0, 3, (rows,), generator=g)]
    fin_tok = torch.randint(4, 1000, (rows, stride), generator=g, dtype=torch.int32)
    for s in range(n):   # slots past fin_count must not be read
        fin_len[s * beam + int(fin_count[s]):(s + 1) * beam] = 1 << 20
        fin_score[s * beam + int(fin_count[s]):(s + 1) * beam] = math.nan
        fin_tok[s * beam + int(fin_count[s]):(s + 1) * beam] = SENT
    a = dict(tok=_ints(rows), cum=_nans(rows), nactive=_ints(n), done=_ints(n), ndone=_ints(1), parent=_ints(rows), new_tok=_ints(rows),
             new_cum=_nans(rows), fin_tok=fin_tok.cuda(), fin_len=fin_len.cuda(), fin_score=fin_score.cuda(), fin_count=fin_count.cuda(),
             margins=_nans((n, 2)), anc=_ints((2, rows, stride)), hist=_ints((2, rows, stride)))
    st = _lib.smi_beam_state(**{k: a[k].data_ptr() for k in a if k not in ("anc", "hist")}, n=n, beam=beam, stride=stride)
    for i in range(2):
        st.anc[i], st.hist[i] = a["anc"][i].data_ptr(), a["hist"][i].data_ptr()
    before = {k: v.cpu() for k, v in a.items()}
    outs = []
    for _ in range(2):
        out = dict(tok=_ints((rows, out_stride)), len=_ints(rows), score=_nans(rows))
        a["margins"].fill_(math.nan)
        _lib.check(lib.smi_beam_output(C.byref(st), out_stride, out["tok"].data_ptr(), out["len"].data_ptr(), out["score"].data_ptr(),
                                       _stream()))
        torch.cuda.synchronize()
        outs.append({**{k: v.cpu() for k, v in out.items()}, "margins": a["margins"].cpu()})
    got = outs[0]
    for s in range(n):
        cnt = int(fin_count[s])
        order = sorted(range(cnt), key=lambda i: -fin_score[s * beam + i].item())          # Python's sort is stable
        for hslot in range(beam):
            row = s * beam + hslot
            if hslot < cnt:
                src = s * beam + order[hslot]
                ln = int(fin_len[src])
                assert got["len"][row].item() == ln and _same_bits(got["score"][row], fin_score[src]), (s, hslot)
                assert torch.equal(got["tok"][row, :ln], fin_tok[src, :ln]) and (got["tok"][row, ln:] == -1).all(), (s, hslot)
            else:   # the empty-slot fill
                assert got["len"][row].item() == 0 and got["score"][row].item() == -math.inf and (got["tok"][row] == -1).all(), (s, hslot)
        assert math.isnan(got["margins"][s, 0].item())
        if cnt >= 2:
            assert _same_bits(got["margins"][s, 1], got["score"][s * beam] - got["score"][s * beam + 1])
        else:
            assert math.isnan(got["margins"][s, 1].item())
    for k in before:
        if k != "margins":
            assert _same_bits(a[k].cpu(), before[k]), k
    for k in got:
        assert _same_bits(got[k], outs[1][k]), k


# ---------------------------------------------------------------------------------------------------- selection alone
def _selection_inputs(rows, vocab, seed):
    return torch.stack([R.hash_row(seed, (r,), vocab) for r in range(rows)])


@pytest.mark.parametrize("f16_tm", [False, True], ids=["f32", "f16tm"])
@pytest.mark.parametrize("block_eos", [0, 1])
@pytest.mark.parametrize("pad_idx", [-1, 5])
def test_selection_alone(lib, pad_idx, block_eos, f16_tm):
    rows, vocab, k2, eos, unk = 7, 5000, 6, 3, 1
    raw = _selection_inputs(rows, vocab, 11)
    # the masked ids hold the row's largest values: a mask that is not applied shows at once
    raw[:, 5] = 9.0
    raw[:, eos] = 8.75
    raw[:, unk] = 8.5
    raw[1, 5:] = -math.inf      # fewer finite candidates than k2
    raw[2, 300] = raw[2, 4100] = raw[2, 4101] = 8.25   # equal values across tiles: the lower token first
    inv_temp = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(1.6, dtype=torch.float32))
    scaled = raw * torch.tensor(inv_temp, dtype=torch.float32)
    dev, ldl = _upload_logits(raw, vocab, f16_tm)
    tile_max, tile_sum = _tile_stats(scaled, vocab)
    outs = []
    for _ in range(2):
        out = dict(pmax=_nans(rows), psum=_nans(rows), pval=_nans((rows, 16)), pidx=_ints((rows, 16)))
        _select(lib, dev, ldl, f16_tm, rows, vocab, tile_max, tile_sum, k2, inv_temp, pad_idx, eos, unk, 1.0, block_eos, out)
        outs.append({k: v.cpu() for k, v in out.items()})
    got = outs[0]
    for r in range(rows):
        ev, ei = _expected_list(scaled[r], k2, pad_idx, eos, unk, 1.0, block_eos)
        assert torch.equal(got["pidx"][r, :k2], ei) and _same_bits(got["pval"][r, :k2], ev), (r, got["pidx"][r], ei)
        assert (got["pidx"][r, k2:] == SENT).all() and torch.isnan(got["pval"][r, k2:]).all()
        assert _same_bits(got["pmax"][r], scaled[r].max())
        finite = scaled[r][torch.isfinite(scaled[r])].double()
        true_sum = torch.exp(finite - finite.max()).sum().item()
        assert abs(got["psum"][r].item() - true_sum) <= 0.5 * R.L_LOG * true_sum
    assert (got["pidx"][1, :k2] == INT_MAX).sum() >= 1 and (5 in got["pidx"][0].tolist()) == (pad_idx != 5)
    assert (eos in got["pidx"][0].tolist()) == (not block_eos)
    for k in got:
        assert _same_bits(got[k], outs[1][k]), k
    # k2 = 0: the normaliser only
    out = dict(pmax=_nans(rows), psum=_nans(rows), pval=_nans((rows, 16)), pidx=_ints((rows, 16)))
    _select(lib, dev, ldl, f16_tm, rows, vocab, tile_max, tile_sum, 0, inv_temp, pad_idx, eos, unk, 1.0, block_eos, out)
    assert _same_bits(out["pmax"].cpu(), got["pmax"]) and _same_bits(out["psum"].cpu(), got["psum"])
    assert torch.isnan(out["pval"]).all() and (out["pidx"] == SENT).all()


@pytest.mark.parametrize("f16_tm", [False, True], ids=["f32", "f16tm"])
def test_selection_table_exit(lib, f16_tm):
    """With the table a row follows its own sentence: forced sentences (prompt token, forced EOS, past the cap) get the normaliser
    only, free ones their list with their own block_eos."""
    n, group, vocab, k2, eos = 5, 2, 1000, 4, 3
    rows = n * group
    lens = [1, 3, 1, 2, 1]
    tok = torch.full((n, 3), 7, dtype=torch.int32)
    tab = dict(tok=tok.cuda(), len=torch.tensor(lens, dtype=torch.int32).cuda(), stride=3, gen_cap=3, min_gen=1, model_max=4)
    plans = [R.Plan((7,) * ln, 3, 1, 4) for ln in lens]
    raw = _selection_inputs(rows, vocab, 12)
    raw[:, eos] = 9.0
    dev, ldl = _upload_logits(raw, vocab, f16_tm)
    tile_max, tile_sum = _tile_stats(raw, vocab)
    seen = set()
    for step_nr in (1, 2, 3, 4):
        out = dict(pmax=_nans(rows), psum=_nans(rows), pval=_nans((rows, 16)), pidx=_ints((rows, 16)))
        # the scalar block_eos is the opposite of what most sentences need: the table's must win
        _select(lib, dev, ldl, f16_tm, rows, vocab, tile_max, tile_sum, k2, 1.0, 0, eos, 1, 0.0, step_nr >= 2, out, tab=tab, group=group,
                step_nr=step_nr)
        got = {k: v.cpu() for k, v in out.items()}
        for r in range(rows):
            p = plans[r // group]
            mode = p.mode(step_nr)
            seen.add((mode, mode == "free" and step_nr < p.min_len))
            assert _same_bits(got["pmax"][r], raw[r].max())
            if mode == "free":
                ev, ei = _expected_list(raw[r], k2, 0, eos, 1, 0.0, step_nr < p.min_len)
                assert torch.equal(got["pidx"][r, :k2], ei) and _same_bits(got["pval"][r, :k2], ev), (step_nr, r)
            else:
                assert torch.isnan(got["pval"][r]).all() and (got["pidx"][r] == SENT).all(), (step_nr, r)
    assert seen == {("prompt", False), ("eos", False), ("past", False), ("free", True), ("free", False)}


def test_special_ids_outside_tile_zero_are_refused(lib):
    """Four tiles, k2 = 2, EOS = 300 blocked and the maximum of tile 1: the tiles read would be 0, 1 and 2 and the list (5, 1) where
    (5, 3) is right.  The selection's tile argument needs the masked ids in tile 0; the entries refuse anything else."""
    from sonar_amd import _lib

    vocab = 1000
    raw = torch.full((1, vocab), -5.0)
    raw[0, 256:512] = 0.0
    raw[0, 300] = 10.0
    raw[0, 512], raw[0, 513] = 5.0, 1.0
    raw[0, 768] = 3.0
    dev, ldl = _upload_logits(raw, vocab, False)
    tile_max, tile_sum = _tile_stats(raw, vocab)
    out = dict(pmax=_nans(1), psum=_nans(1), pval=_nans((1, 16)), pidx=_ints((1, 16)))
    for ids in (dict(pad=0, eos=300, unk=1), dict(pad=300, eos=3, unk=1), dict(pad=0, eos=3, unk=300)):
        with pytest.raises(_lib.SmiError, match="below 256"):
            _select(lib, dev, ldl, False, 1, vocab, tile_max, tile_sum, 2, 1.0, ids["pad"], ids["eos"], ids["unk"], 0.0, 1, out)
        assert torch.isnan(out["pval"]).all() and (out["pidx"] == SENT).all()   # nothing ran
    # the same row with the special ids where they belong: the list is the right one
    _select(lib, dev, ldl, False, 1, vocab, tile_max, tile_sum, 2, 1.0, 0, 3, 1, 0.0, 1, out)
    assert out["pidx"][0, :2].tolist() == [300, 512] and out["pval"][0, :2].tolist() == [10.0, 5.0]
    raw[0, 300] = -5.0
    dev, ldl = _upload_logits(raw, vocab, False)
    tile_max, tile_sum = _tile_stats(raw, vocab)
    _select(lib, dev, ldl, False, 1, vocab, tile_max, tile_sum, 2, 1.0, 0, 3, 1, 0.0, 1, out)
    assert out["pidx"][0, :2].tolist() == [512, 768] and out["pval"][0, :2].tolist() == [5.0, 3.0]
