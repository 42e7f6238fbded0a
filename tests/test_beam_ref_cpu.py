"""CPU: the restatement of the beam search's bookkeeping (tests/beam_ref.py) equals the oracle's beam search bit for bit, the
inputs of the kernel tests (tests/test_gpu_beam_kernels.py) satisfy the gap condition that replaces the near-tie excuse and meet the
situations they were built for, and the new C-ABI entries refuse bad arguments before the device is asked for."""
import ctypes as C
import dataclasses
import math

import pytest
import torch

from oracle import text_decoder as OD
from tests import beam_ref as R

INVALID_ARG, UNSUPPORTED, NO_DEVICE = -1, -2, -3


# --------------------------------------------------------------------------------------------------- (a) against the oracle
@pytest.mark.parametrize("beam", [1, 3, 5])
def test_search_equals_the_oracle_beam_search(beam):
    cfg = OD.OracleTextDecoderConfig(model_dim=64, num_layers=2, num_heads=4, ffn_inner_dim=128, vocab_size=120, max_seq_len=64)
    params = OD.make_synthetic_params(cfg, seed=6, std=0.3)
    emb = torch.randn(3, 64, generator=torch.Generator().manual_seed(2))
    prompt = [3, 60]
    want = OD.beam_search(params, cfg, emb, prompt, beam_size=beam, max_gen_len=(0, 7))

    class Logits:   # the oracle runs a sentence's live rows as one batch
        def batch(self, s, hists):
            return OD.decoder_logits(params, cfg, emb[s:s + 1].expand(len(hists), -1), torch.tensor(hists))[:, -1]

    got = R.search(R.BeamParams(beam), [R.Plan(tuple(prompt), 7, 1, cfg.max_seq_len)] * 3, Logits(), dtype=torch.float32)
    for w, g in zip(want, got.hyps):
        assert [h.seq.tolist() for h in w] == [t for t, _ in g]
        assert [h.score for h in w] == [sc for _, sc in g]      # the same bits, in the same order
    assert all(len(g) == beam for g in got.hyps)


def test_plan_modes_are_those_of_the_device_table():
    p = R.Plan((3, 7, 9), gen_cap=4, min_gen=2, model_max=6)
    assert (p.plen, p.max_len, p.min_len) == (3, 6, 5)
    assert [p.mode(k) for k in range(1, 8)] == ["prompt", "prompt", "free", "free", "eos", "past", "past"]
    p = R.Plan((3,), gen_cap=1)
    assert p.max_len == 2 and p.mode(1) == "eos"


# -------------------------------------------------------------------------------------------------- (b) the rules, by hand
def _row(vocab=12, **vals):
    row = torch.full((vocab,), -20.0)
    for k, v in vals.items():
        row[int(k[1:])] = v
    return row


def test_step_eos_rules_tie_order_and_margin():
    P = R.BeamParams(beam=2)
    plan = R.Plan((3,), gen_cap=10)
    # two rows with identical logits and identical cum: an exact tie, resolved row first, then token
    lg = torch.stack([_row(t5=2.0, t6=2.0, t3=1.0, t7=0.0)] * 2)
    o = R.step(P, plan, 3, [R.Row([3, 5, 5], -1.0), R.Row([3, 5, 6], -1.0)], lg, nfin=0)
    assert [(r, t) for _, r, t in o.ranked] == [(0, 5), (0, 6), (1, 5), (1, 6)]
    assert o.cont[0][:2] == (0, 5) and o.cont[1][:2] == (0, 6) and not o.fin and not o.done
    assert o.margin == 0.0 and len(o.gaps) == 2 and all(g.by_construction and g.gap == 0.0 for g in o.gaps)
    o = R.step(P, plan, 3, [R.Row([3, 5, 5], -1.0), R.Row([3, 5, 6], -1.0 - 1e-9)], lg, nfin=0)
    assert [(r, t) for _, r, t in o.ranked] == [(0, 5), (0, 6), (1, 5), (1, 6)] and not o.gaps[1].by_construction
    assert R.gap_violations(o.gaps, R.G_GAP) == [o.gaps[1]]       # a near-tie that is none by construction breaks the condition
    assert [le for le in o.lists[0][1]] == [5, 6, 3, 7]
    # EOS second of four: it finishes (rank < beam); EOS third: it neither finishes nor continues
    lg = torch.stack([_row(t5=3.0, t3=2.5, t6=2.0, t7=1.0)])
    o = R.step(P, plan, 3, [R.Row([3, 5, 5], 0.0)], lg, nfin=0)
    assert [t for _, _, t in o.ranked] == [5, 3, 6, 7] and [f[0] for f in o.fin] == [0] and [c[1] for c in o.cont] == [5, 6]
    assert o.fin[0][2] == pytest.approx(o.fin[0][1] / 3)          # seq_len - 1 = step_nr
    lg = torch.stack([_row(t5=3.0, t6=2.5, t3=2.0, t7=1.0)])
    o = R.step(P, plan, 3, [R.Row([3, 5, 5], 0.0)], lg, nfin=0)
    assert not o.fin and [c[1] for c in o.cont] == [5, 6] and "EOS between beam and 2 beam" in o.events
    assert len(o.gaps) == 2                                        # (5, 6) and (6, EOS): 7 decides nothing
    # the hypothesis that completes the beam ends the sentence at once
    lg = torch.stack([_row(t3=3.0, t5=2.5, t6=2.0, t7=1.0)])
    o = R.step(P, plan, 3, [R.Row([3, 5, 5], 0.0)], lg, nfin=1)
    assert o.done and not o.cont and len(o.fin) == 1 and len(o.gaps) == 1 and "beam completed mid-list" in o.events
    # PAD never, UNK penalised, EOS blocked below min_len, -inf is no candidate
    lg = torch.stack([_row(t0=9.0, t1=3.0, t3=8.0, t5=2.0, t6=-math.inf)])
    lg[0, 7:] = -math.inf
    o = R.step(R.BeamParams(beam=3, unk_penalty=2.0), R.Plan((3,), 10, min_gen=5), 2, [R.Row([3, 5], 0.0)], lg, nfin=0)
    assert [t for _, _, t in o.ranked] == [5, 1, 2, 4] and len(o.cont) == 3 and o.lists[0][0][1] == pytest.approx(1.0)
    # forced steps
    o = R.step(P, R.Plan((3, 7, 9), 4), 2, [R.Row([3, 7], -1.0)], torch.stack([_row(t9=1.0)]), nfin=0)
    assert o.kind == "prompt" and o.cont[0][:2] == (0, 9)
    o = R.step(P, R.Plan((3,), 3), 3, [R.Row([3, 5, 5], -1.0), R.Row([3, 5, 6], -0.5)], torch.stack([_row(t3=1.0)] * 2), nfin=1)
    assert o.kind == "eos" and o.done and [f[0] for f in o.fin] == [1]


def test_len_penalty_and_normalize():
    lg = torch.stack([_row(t3=3.0, t5=2.5)])
    for lp, norm, div in ((0.5, True, 4 ** 0.5), (2.0, True, 16.0), (1.0, False, 1.0)):
        o = R.step(R.BeamParams(beam=1, len_penalty=lp, normalize=norm), R.Plan((3,), 10), 4, [R.Row([3, 5, 5, 5], -2.0)], lg, nfin=0)
        assert o.fin[0][2] == pytest.approx(o.fin[0][1] / div)


# ------------------------------------------------------------------------------------------ (c) the inputs of the kernel tests
def test_hash_rows_are_fp16_exact_quarter_steps():
    a, b = R.hash_row(1, (0, 3, 5), 5000), R.hash_row(1, (0, 3, 5), 5000)
    assert torch.equal(a, b) and not torch.equal(a, R.hash_row(1, (0, 3, 6), 5000)) and not torch.equal(a, R.hash_row(2, (0, 3, 5), 5000))
    assert a.dtype == torch.float32 and torch.equal(a.half().float(), a) and torch.equal((a * 4).round() / 4, a)
    assert a.min() >= -8 and a.max() <= 8 and a.max() >= 7
    top = torch.sort(a[:1000], descending=True).values[:10]
    assert 2 <= len(top.unique()) <= 10                            # ties and gaps among a row's best
    S = R.Synthetic(1, 1000, by_position=True, dup=(10, 300, 700))
    r = S(0, [3, 5])
    assert torch.equal(r, S(0, [3, 9])) and not torch.equal(r, S(1, [3, 5])) and (r[[10, 300, 700]] == r.max()).all()
    d = R.Synthetic(1, 1000, descending=4)(0, [3, 6])
    assert torch.isfinite(d).nonzero().flatten().tolist() == [0, 3, 4, 5]


@pytest.fixture(scope="module")
def searches():
    return {name: R.search(c.P, c.plans, c.logits) for name, c in R.CASES.items()}


def test_error_model_constants():
    assert R.B_STEP == 1.5 * 2.0 ** -17 + 3 * 2.0 ** -23 * 16 + R.L_LOG and R.G_GAP == 16 * R.B_STEP
    assert 1e-4 < R.G_GAP < 1e-3


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_satisfies_the_gap_condition(searches, name):
    """Every pair of neighbours inside a decision range is tied by construction or at least G apart, the final ranking's included:
    with it no rounding of the device can reorder them, and the GPU test excuses nothing."""
    o = searches[name]
    assert o.max_abs_cum <= R.CUM_MAX
    ngaps = 0
    for s, gaps in enumerate(o.gaps):
        bad = R.gap_violations(gaps, R.G_GAP)
        assert not bad, (name, s, bad[:3])
        ngaps += len(gaps)
    assert ngaps >= 4 * len(o.gaps)
    beam = R.CASES[name].P.beam
    assert all(len(h) == beam for h in o.hyps)                     # every sentence collects its `beam` hypotheses


def test_cases_meet_what_they_were_built_for(searches):
    for name in ("eos_pressure_beam3", "eos_pressure_beam5"):
        assert {"several rows finish", "beam completed mid-list", "EOS between beam and 2 beam"} <= searches[name].events, name
        assert len({len(h[0][0]) for h in searches[name].hyps}) >= 3   # sentences end at different positions: inert rows next to live ones
    for name in ("ties_beam3", "ties_beam5"):
        o = searches[name]
        ties = [g for gs in o.gaps for g in gs if g.by_construction]
        assert len(ties) >= 10 * len(o.gaps), name
        # tied EOS candidates of sibling rows, one EOS left over when the beam is complete, equal finished scores
        assert {"several rows finish", "beam completed mid-list"} <= o.events, name
        assert any(g.by_construction and g.where == "final ranking" for gs in o.gaps for g in gs), name
    for name in ("few_finite_beam5", "few_finite_beam8"):
        o, beam = searches[name], R.CASES[name].P.beam
        assert any(n[0] < beam for n in o.nactive), name            # fewer candidates than the beam
        assert any(b < a for n in o.nactive for a, b in zip(n, n[1:])), name   # the live rows shrink
    t = R.CASES["table_beam3"]
    assert sorted({p.plen for p in t.plans}) == [1, 2, 4] and len({p.max_len for p in t.plans}) == 3
    assert any(len(h[-1][0]) == p.max_len - p.plen for h, p in zip(searches["table_beam3"].hyps, t.plans))   # forced EOS at the cap
    e = R.CASES["table_equal_lengths_beam2"]
    assert len({p.plen for p in e.plans}) == 1 and len({p.prompt for p in e.plans}) == len(e.plans)
    assert any(tok >= 256 for tok in R.CASES["prompt3_beam3"].plans[0].prompt[1:])   # forced tokens outside tile 0


def test_unk_penalty_cases_move_unk_across_the_list():
    for name, inside_without, inside_with in (("unk_plus2", True, False), ("unk_minus2", False, True)):
        c = R.CASES[name]
        seen = {False: [], True: []}
        for with_pen in (False, True):
            P = c.P if with_pen else dataclasses.replace(c.P, unk_penalty=0.0)
            for s in range(len(c.plans)):
                o = R.step(P, c.plans[s], 1, [R.Row([3], 0.0)], c.logits(s, [3])[None], nfin=0)
                seen[with_pen].append(P.unk_idx in o.lists[0][1])
        assert all(v == inside_without for v in seen[False]) and all(v == inside_with for v in seen[True]), (name, seen)


# --------------------------------------------------------------------------------------------------------- (d) refusals
@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _good(_lib):
    p = 0x1000   # never dereferenced: every call below is refused
    table = dict(tok=None, len=None, stride=0, gen_cap=0, min_gen=0, model_max=0)
    sel = dict(logits=p, ldl=1024, logits_f16_tm=0, rows=15, vocab=1000, tile_max=p, tile_sum=p, stat_rows=15, k2=6, inv_temp=1.0,
               pad_idx=0, eos_idx=3, unk_idx=1, unk_penalty=0.0, block_eos=0, pmax=p, psum=p, pval=p, pidx=p, group=3, step_nr=1)
    st = dict({k: p for k in ("tok", "cum", "nactive", "done", "ndone", "parent", "new_tok", "new_cum", "fin_tok", "fin_len",
                              "fin_score", "fin_count", "margins")}, anc=(p, p), hist=(p, p), n=5, beam=3, stride=12)
    step = dict(logits=p, ldl=1024, logits_f16_tm=0, vocab=1000, pmax=p, psum=p, pval=p, pidx=p, k2=6, pos=4, prompt_len=1,
                forced_tok=-1, max_len=12, inv_temp=1.0, len_penalty=1.0, normalize=1, eos_idx=3)
    return table, sel, st, step


def _call(lib, _lib, name, table, sel, st, step, extra):
    tab = _lib.smi_prompt_table(**table)
    state = _lib.smi_beam_state(**{k: v for k, v in st.items() if k not in ("anc", "hist")})
    state.anc[0], state.anc[1] = st["anc"]
    state.hist[0], state.hist[1] = st["hist"]
    if name == "smi_vocab_select":
        return lib.smi_vocab_select(C.byref(_lib.smi_vocab_select_args(table=tab, **sel)), None)
    if name == "smi_beam_step":
        return lib.smi_beam_step(C.byref(state), C.byref(_lib.smi_beam_step_args(table=tab, **step)), None)
    if name == "smi_beam_init":
        return lib.smi_beam_init(C.byref(state), extra.get("first_tok", 3), extra.get("first_toks"), extra.get("first_stride", 0), None)
    if name == "smi_beam_reorder":
        return lib.smi_beam_reorder(C.byref(state), extra.get("pos", 4), None)
    return lib.smi_beam_output(C.byref(state), extra.get("out_stride", 11), extra.get("out_tok", 0x1000), extra.get("out_len", 0x1000),
                               extra.get("out_score", 0x1000), None)


def test_refusals_need_no_device(lib):
    from sonar_amd import _lib

    if lib.smi_device_count() > 0:
        pytest.skip("a HIP device is visible: the made-up pointers must never reach a kernel")
    A, U = INVALID_ARG, UNSUPPORTED
    tab_on = dict(tok=0x1000, len=0x1000, stride=4, gen_cap=6, min_gen=1, model_max=12)
    # (entry, which argument group, change, code, text)
    cases = [("smi_vocab_select", "sel", {k: None}, A, "null argument") for k in ("logits", "tile_max", "tile_sum", "pmax", "psum", "pval", "pidx")]
    cases += [
        ("smi_vocab_select", "sel", {"ldl": 1000}, A, "multiple of 256"), ("smi_vocab_select", "sel", {"vocab": 1025}, A, "multiple of 256"),
        ("smi_vocab_select", "sel", {"rows": 0}, A, "multiple of 256"),
        ("smi_vocab_select", "sel", {"stat_rows": 14}, A, "stat_rows"), ("smi_vocab_select", "sel", {"k2": 17}, A, "k2 17"),
        ("smi_vocab_select", "sel", {"k2": -1}, A, "k2 -1"), ("smi_vocab_select", "sel", {"inv_temp": 0.0}, A, "inv_temp"),
        ("smi_vocab_select", "sel", {"unk_penalty": math.inf}, A, "unk_penalty"),
        ("smi_vocab_select", "sel", {"pad_idx": -2}, A, "bad special ids"),
        # the special ids live in tile 0: the tile argument of the selection depends on it
        ("smi_vocab_select", "sel", {"eos_idx": 300}, U, "below 256"), ("smi_vocab_select", "sel", {"pad_idx": 256}, U, "below 256"),
        ("smi_vocab_select", "sel", {"unk_idx": 999}, U, "below 256"), ("smi_vocab_select", "sel", {"vocab": 100, "ldl": 256, "eos_idx": 100}, U, "below 256"),
        ("smi_vocab_select", "table", {**tab_on, "len": None}, A, "without lengths"),
        ("smi_vocab_select", "table", {**tab_on, "gen_cap": 0}, A, "gen_cap=0"), ("smi_vocab_select", "table", {**tab_on, "stride": 0}, A, "stride=0"),
        ("smi_vocab_select", "table+sel", ({**tab_on}, {"group": 4}), A, "group=4"),
        ("smi_vocab_select", "table+sel", ({**tab_on}, {"step_nr": 0}), A, "step_nr=0"),
    ]
    for entry in ("smi_beam_init", "smi_beam_step", "smi_beam_reorder", "smi_beam_output"):
        cases += [(entry, "st", {k: None}, A, "null argument") for k in ("tok", "ndone", "new_cum", "fin_tok", "fin_count")]
        cases += [(entry, "st", {"anc": (0x1000, None)}, A, "null argument"), (entry, "st", {"hist": (None, 0x1000)}, A, "null argument"),
                  (entry, "st", {"beam": 9}, A, "beam=9"), (entry, "st", {"beam": 0}, A, "beam=0"), (entry, "st", {"n": 0}, A, "n=0"),
                  (entry, "st", {"stride": 1}, A, "stride=1")]
    cases += [("smi_beam_step", "step", {k: None}, A, "null argument") for k in ("logits", "pmax", "psum", "pval", "pidx")]
    cases += [
        ("smi_beam_step", "step", {"k2": 5}, A, "k2=5 must be 2 * beam=3"), ("smi_beam_step", "step", {"pos": 11}, A, "pos=11"),
        ("smi_beam_step", "step", {"pos": -1}, A, "pos=-1"), ("smi_beam_step", "step", {"ldl": 512}, A, "multiple of 256"),
        ("smi_beam_step", "step", {"inv_temp": -1.0}, A, "inv_temp"), ("smi_beam_step", "step", {"eos_idx": -1}, A, "eos_idx=-1"),
        ("smi_beam_step", "step", {"eos_idx": 1000}, A, "eos_idx=1000"), ("smi_beam_step", "step", {"prompt_len": 0}, A, "prompt_len=0"),
        ("smi_beam_step", "step", {"prompt_len": 8, "forced_tok": 1000}, A, "forced_tok=1000"),
        ("smi_beam_step", "step", {"prompt_len": 8, "forced_tok": -1}, A, "forced_tok=-1"),
        ("smi_beam_step", "step", {"max_len": 5}, A, "past the forced EOS"), ("smi_beam_step", "table", {**tab_on, "model_max": 1}, A, "model_max=1"),
        ("smi_beam_init", "extra", {"first_tok": -1}, A, "first_tok=-1"), ("smi_beam_init", "extra", {"first_toks": 0x1000, "first_stride": 0}, A, "first_stride=0"),
        ("smi_beam_reorder", "extra", {"pos": 11}, A, "pos=11"), ("smi_beam_reorder", "extra", {"pos": -1}, A, "pos=-1"),
        ("smi_beam_output", "extra", {"out_stride": 0}, A, "out_stride=0"), ("smi_beam_output", "extra", {"out_tok": None}, A, "null argument"),
        ("smi_beam_output", "extra", {"out_score": None}, A, "null argument"),
    ]
    wrong = []
    for entry, group, change, code, text in cases:
        table, sel, st, step = _good(_lib)
        extra = {}
        parts = {"table": table, "sel": sel, "st": st, "step": step, "extra": extra}
        for g, ch in zip(group.split("+"), change if isinstance(change, tuple) else (change,)):
            assert g == "extra" or set(ch) <= set(parts[g]), (entry, ch)
            parts[g].update(ch)
        rc = _call(lib, _lib, entry, table, sel, st, step, extra)
        err = lib.smi_last_error().decode()
        if rc != code or text not in err:
            wrong.append((entry, change, code, text, rc, err))
    assert not wrong, wrong
    # the unchanged calls pass every check and stop at the device; so do the forms that are no refusals
    ok = [(e, "extra", {}) for e in ("smi_vocab_select", "smi_beam_init", "smi_beam_step", "smi_beam_reorder", "smi_beam_output")]
    ok += [("smi_vocab_select", "sel", {"k2": 0}), ("smi_vocab_select", "sel", {"pad_idx": -1, "eos_idx": -1, "unk_idx": -1}),
           ("smi_vocab_select", "sel", {"eos_idx": 255}), ("smi_vocab_select", "sel", {"logits_f16_tm": 1}),
           ("smi_vocab_select", "table", tab_on), ("smi_beam_step", "table", tab_on), ("smi_beam_step", "st", {"margins": None}),
           ("smi_beam_step", "step", {"logits_f16_tm": 1}), ("smi_beam_step", "step", {"pos": 10, "max_len": 12}),
           ("smi_beam_init", "extra", {"first_toks": 0x1000, "first_stride": 4}), ("smi_beam_reorder", "extra", {"pos": 0})]
    for entry, group, change in ok:
        table, sel, st, step = _good(_lib)
        extra = {}
        {"table": table, "sel": sel, "st": st, "step": step, "extra": extra}[group].update(change)
        rc = _call(lib, _lib, entry, table, sel, st, step, extra)
        assert rc == NO_DEVICE and "no HIP device visible" in lib.smi_last_error().decode(), (entry, change, rc, lib.smi_last_error())
    assert lib.smi_abi_version() == 7   # the entry points are additions


def test_special_ids_above_tile_zero_are_refused_everywhere(lib):
    """The tile argument of the selection needs PAD, EOS and UNK among the ids 0..255: decoder create and both
    selection entries refuse anything else, before the device is asked for."""
    from sonar_amd import _lib

    if lib.smi_device_count() > 0:
        pytest.skip("a HIP device is visible: the made-up pointers must never reach a kernel")
    base = dict(model_dim=256, num_layers=1, num_heads=4, ffn_inner_dim=512, vocab_size=1000, max_seq_len=32, pos_offset=2,
                input_dim=256, embed_scale=16.0, ln_eps=1e-5, pad_idx=0, unk_idx=1, bos_idx=2, eos_idx=3)
    w = _lib.smi_text_decoder_weights()
    out = C.c_void_p()
    for change, code, text in (({"eos_idx": 300}, UNSUPPORTED, "below 256"), ({"pad_idx": 256}, UNSUPPORTED, "below 256"),
                               ({"unk_idx": 700}, UNSUPPORTED, "below 256"), ({"eos_idx": -1}, INVALID_ARG, "bad special ids"),
                               ({"vocab_size": 100, "unk_idx": 100}, UNSUPPORTED, "below 256")):
        cfg = _lib.smi_text_decoder_config(**{**base, **change})
        rc = lib.smi_text_decoder_create(C.byref(cfg), C.byref(w), C.byref(out))
        assert rc == code and text in lib.smi_last_error().decode(), (change, rc, lib.smi_last_error())
    sp, keep = _lib.step_processors_struct(1, ())
    p = 0x1000
    for pad, code, text in ((256, UNSUPPORTED, "below 256"), (999, UNSUPPORTED, "below 256"), (-2, INVALID_ARG, "bad special ids"),
                            (5, NO_DEVICE, "no HIP device"), (-1, NO_DEVICE, "no HIP device")):
        rc = lib.smi_vocab_select_banned(p, 1024, 0, 4, 1000, p, p, 6, pad, p, 8, 8, C.byref(sp), p, p, p, p, None)
        assert rc == code and text in lib.smi_last_error().decode(), (pad, rc, lib.smi_last_error())
    del keep
