"""GPU: per-sentence prompts of the on-device decoding (smi_text_decoder_generate_prompts / _sample_prompts).

The whole specification is row independence: row i of a call with per-sentence prompts returns what the one-prompt call
with prompt p_i returns for that row (same row count, hence the same engines and chains: INTEGRATION.md 6).  That is tested
bit for bit against today's entry, and against the CPU oracle, which already is a per-sentence loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS_REL = 1e-3
N = 40
GEN = (0, 13)


def _cfgs(d=256, heads=4, ffn=512, layers=2, vocab=1000, max_seq_len=64):
    from oracle.text_decoder import OracleTextDecoderConfig
    from sonar_amd.text_decoder import SonarTextDecoderConfig
    from sonar_amd.text_encoder import VocabularyInfo

    o = OracleTextDecoderConfig(model_dim=d, num_layers=layers, num_heads=heads, ffn_inner_dim=ffn,
                                vocab_size=vocab, max_seq_len=max_seq_len)
    c = SonarTextDecoderConfig(model_dim=d, num_decoder_layers=layers, num_decoder_attn_heads=heads,
                               ffn_inner_dim=ffn, vocab_info=VocabularyInfo(size=vocab), max_seq_len=max_seq_len)
    return o, c


@pytest.fixture(scope="module")
def setup():
    from oracle import text_decoder as OD
    from sonar_amd.text_decoder import TextDecoderEngine

    ocfg, cfg = _cfgs()
    params = OD.make_synthetic_params(ocfg, seed=4321, std=0.09)
    eng = TextDecoderEngine(cfg, params, device="cuda:0")
    return OD, ocfg, params, eng


@pytest.fixture(scope="module")
def toy():
    """The generic-dimension (flex) path: d 32, 4 heads of 8."""
    from oracle import text_decoder as OD
    from sonar_amd.text_decoder import TextDecoderEngine

    ocfg, cfg = _cfgs(d=32, heads=4, ffn=128, vocab=1024)
    params = OD.make_synthetic_params(ocfg, seed=11, std=0.3)
    eng = TextDecoderEngine(cfg, params, device="cuda:0", dtype=torch.float32)
    return OD, ocfg, params, eng


def prompts_for(n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        extra = [0, 0, 1, 2, 4][i % 5]                     # forced-prefix tokens after [</s>, lang]
        lang = 700 + int(torch.randint(0, 8, (1,), generator=g))
        out.append([3, lang] + [int(t) for t in torch.randint(4, 1000, (extra,), generator=g)])
    return out


def _inputs(beam, dim=256):
    emb = torch.randn(N, dim, generator=torch.Generator().manual_seed(310 + beam)) * 0.3
    return emb, prompts_for(N, 320 + beam)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_rows_equal(mixed, single, rows, what):
    """mixed / single: tuples of device tensors [n, ...]; single's token rows may be narrower (its own max_len): the mixed
    row must hold the same tokens there and -1 beyond."""
    mt, st = mixed[0].cpu(), single[0].cpu()
    L = st.shape[-1]
    assert mt.shape[-1] >= L
    for i in rows:
        assert torch.equal(mixed[1][i].cpu(), single[1][i].cpu()), f"{what}: lens of row {i}"
        assert torch.equal(mt[i][..., :L], st[i]), f"{what}: tokens of row {i}"
        assert (mt[i][..., L:] == -1).all(), f"{what}: row {i} is not -1 padded past its own width"
        for k in range(2, len(single)):   # scores, margins: bit for bit
            assert torch.equal(_bits(mixed[k][i]), _bits(single[k][i])), (
                f"{what}: output {k} of row {i}: {mixed[k][i].tolist()} vs {single[k][i].tolist()}")


def _check_independence(eng, emb, prompts, what, sample=None, **kw):
    """Row i of the per-sentence call == row i of the one-prompt call with prompts[i] on ALL the embeddings."""
    n = emb.shape[0]
    e = emb.cuda()

    def call(p):
        if sample is None:
            t, l, s = eng.generate(e, p, **kw)
            return t, l, s, eng.last_margins(n)
        return eng.sample(e, p, sample, **kw)

    mixed = call(prompts)
    torch.cuda.synchronize()
    distinct = []
    for p in prompts:
        if p not in distinct:
            distinct.append(p)
    checked = 0
    for p in distinct:
        rows = [i for i in range(n) if prompts[i] == p]
        _assert_rows_equal(mixed, call(p), rows, f"{what}, prompt {p}")
        checked += len(rows)
    assert checked == n
    return mixed


# ------------------------------------------------------------------------------------------ 1. row independence
@pytest.mark.parametrize("beam", [1, 5])
def test_rows_equal_the_one_prompt_calls(setup, beam):
    _, _, _, eng = setup
    emb, prompts = _inputs(beam)
    assert len({len(p) for p in prompts}) == 4 and len({p[1] for p in prompts}) > 1
    toks, lens, _, _ = _check_independence(eng, emb, prompts, f"beam {beam}", beam_size=beam, max_gen_len=GEN)
    assert toks.shape == (N, beam, max(len(p) for p in prompts) + GEN[1])
    assert (lens.cpu()[:, 0] >= 2).all()


@pytest.mark.parametrize("beam", [1, 5])
def test_rows_equal_with_unk_penalty_and_temperature(setup, beam):
    _, _, _, eng = setup
    emb, prompts = _inputs(beam)
    _check_independence(eng, emb, prompts, f"unk/temperature, beam {beam}", beam_size=beam, max_gen_len=GEN,
                        unk_penalty=0.7, temperature=0.8, min_gen_len=3)


@pytest.mark.parametrize("beam", [1, 5])
def test_rows_equal_under_step_processors(setup, beam):
    from sonar_amd.generation import BannedSequenceProcessor, NGramRepeatBlockProcessor

    _, _, _, eng = setup
    emb, prompts = _inputs(beam)
    # bans that bite: the tokens the unconstrained search likes best after the languages of these prompts
    free = eng.generate(emb.cuda(), prompts, beam_size=1, max_gen_len=GEN)[0].cpu()
    common = torch.bincount(free[free >= 4].flatten()).argsort(descending=True)[:3].tolist()
    procs = [NGramRepeatBlockProcessor(2), BannedSequenceProcessor([(common[0],), (701, common[1]), (common[1], common[2])])]
    _check_independence(eng, emb, prompts, f"step processors, beam {beam}", beam_size=beam, max_gen_len=GEN,
                        step_processors=procs)


@pytest.mark.parametrize("beam", [1, 5])
def test_sampled_rows_equal_the_one_prompt_calls(setup, beam):
    from sonar_amd.generation import BannedSequenceProcessor, NGramRepeatBlockProcessor, TopKSampler, TopPSampler

    _, _, _, eng = setup
    emb, prompts = _inputs(beam)   # (sampling has no beam: the parameter only selects the inputs)
    for sampler in (TopKSampler(6), TopPSampler(0.85)):
        toks, lens, _ = _check_independence(eng, emb, prompts, f"{sampler}", sample=sampler, max_gen_len=GEN, seed=1234 + beam)
        assert toks.shape == (N, max(len(p) for p in prompts) + GEN[1]) and (lens.cpu() >= 1).all()
    _check_independence(eng, emb, prompts, "top-k, unk penalty, min length", sample=TopKSampler(4), max_gen_len=GEN, seed=7,
                        unk_penalty=0.2, temperature=1.3, min_gen_len=4)
    _check_independence(eng, emb, prompts, "top-p under step processors", sample=TopPSampler(0.9), max_gen_len=GEN, seed=9,
                        step_processors=[NGramRepeatBlockProcessor(2), BannedSequenceProcessor([(5,), (701, 17)])])


@pytest.mark.parametrize("beam", [1, 5])
def test_rows_equal_on_the_generic_dimension_path(toy, beam):
    from sonar_amd.generation import NGramRepeatBlockProcessor, TopKSampler

    _, _, _, eng = toy
    emb, prompts = _inputs(beam, dim=32)
    _check_independence(eng, emb, prompts, f"toy, beam {beam}", beam_size=beam, max_gen_len=GEN)
    _check_independence(eng, emb, prompts, f"toy, processors, beam {beam}", beam_size=beam, max_gen_len=GEN,
                        step_processors=[NGramRepeatBlockProcessor(2)], unk_penalty=0.5)
    _check_independence(eng, emb, prompts, "toy, top-k", sample=TopKSampler(5), max_gen_len=GEN, seed=77 + beam)


def test_rows_equal_in_two_chains(setup):
    """160 sentences x beam 5 in two chains of 400 hypothesis rows each: the prompt table is sliced per sentence group."""
    _, ocfg, _, eng = setup
    n = 160
    emb = torch.randn(n, ocfg.model_dim, generator=torch.Generator().manual_seed(333)) * 0.3
    four = [[3, 700], [3, 705], [3, 702, 41], [3, 707, 99, 512, 8]]
    pick = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(334)).tolist()
    prompts = [four[k] for k in pick]
    assert {tuple(p) for p in prompts[:80]} == {tuple(p) for p in prompts[80:]} == {tuple(p) for p in four}
    eng.set_chains(2)
    try:
        _check_independence(eng, emb, prompts, "2 chains", beam_size=5, max_gen_len=(0, 6))
    finally:
        eng.set_chains(0)


# ------------------------------------------------------------------------------------------ 2. all-equal prompts
@pytest.mark.parametrize("beam", [1, 5])
def test_all_equal_prompts_are_the_one_prompt_call(setup, beam):
    from sonar_amd.generation import TopPSampler

    _, _, _, eng = setup
    emb, _ = _inputs(beam)
    e = emb.cuda()
    a = eng.generate(e, [[3, 700]] * N, beam_size=beam, max_gen_len=GEN) + (eng.last_margins(N),)
    b = eng.generate(e, [3, 700], beam_size=beam, max_gen_len=GEN) + (eng.last_margins(N),)
    assert a[0].shape == b[0].shape
    _assert_rows_equal(a, b, range(N), "all-equal prompts")
    a = eng.sample(e, [[3, 700]] * N, TopPSampler(0.9), max_gen_len=GEN, seed=5)
    b = eng.sample(e, [3, 700], TopPSampler(0.9), max_gen_len=GEN, seed=5)
    _assert_rows_equal(a, b, range(N), "all-equal prompts, sampling")


# ------------------------------------------------------------------------------------------ 3. / 4. the oracle
def _logit_range(OD, params, ocfg, emb, prompts):
    """Range of the logits at the prompt positions, every row under its own prompt (rows grouped by prompt length)."""
    lo, hi = float("inf"), float("-inf")
    for plen in sorted({len(p) for p in prompts}):
        rows = [i for i, p in enumerate(prompts) if len(p) == plen]
        lg = OD.decoder_logits(params, ocfg, emb[rows], torch.tensor([prompts[i] for i in rows]))
        lo, hi = min(lo, lg.min().item()), max(hi, lg.max().item())
    return hi - lo


def _rescored(OD, params, ocfg, e, prompt, seq):
    full = torch.tensor([list(prompt) + seq])
    lp = torch.log_softmax(OD.decoder_logits(params, ocfg, e.unsqueeze(0), full[:, :-1]), dim=-1)
    return lp[0, torch.arange(full.shape[1] - 1), full[0, 1:]].sum().item()


def test_greedy_rows_equal_the_oracle(setup):
    """Beam 1: every row's tokens are the oracle's for that row's prompt; no row is excused (the smallest decision or final
    margin the oracle measures over these 40 rows is 0.180, 13 x the 1.37e-2 that 1e-3 of the logit range comes to)."""
    OD, ocfg, params, eng = setup
    emb, prompts = _inputs(1)
    toks, lens, _ = eng.generate(emb.cuda(), prompts, beam_size=1, max_gen_len=GEN)
    toks, lens = toks.cpu(), lens.cpu()
    for i in range(N):
        ref = OD.beam_search_incremental(params, ocfg, emb[i:i + 1], prompts[i], beam_size=1, max_gen_len=GEN)[0][0].seq
        assert toks[i, 0, :int(lens[i, 0])].tolist() == ref.tolist(), f"row {i}, prompt {prompts[i]}"


def test_beam5_rows_against_the_oracle(setup):
    """The rule of tests/test_gpu_decoder.py::test_beam_search_vs_oracle, per row under its own prompt."""
    from tests.neartie import check_engine_margin, oracle_excuses

    OD, ocfg, params, eng = setup
    beam = 5
    emb, prompts = _inputs(beam)
    kw = dict(beam_size=beam, max_gen_len=GEN)
    toks, lens, scores = eng.generate(emb.cuda(), prompts, **kw)
    margins = eng.last_margins(N).cpu()
    toks, lens, scores = toks.cpu(), lens.cpu(), scores.cpu()
    eps = EPS_REL * _logit_range(OD, params, ocfg, emb, prompts)
    excused = []
    for i in range(N):
        prompt = prompts[i]
        om = []
        ref = OD.beam_search_incremental(params, ocfg, emb[i:i + 1], prompt, margins_out=om, **kw)[0]
        L = int(lens[i, 0])
        seq = toks[i, 0, :L].tolist()
        assert L >= 2 and seq[-1] == 3 and 0 not in seq and all(t >= 0 for t in seq)
        assert (toks[i, 0, L:] == -1).all()
        total = _rescored(OD, params, ocfg, emb[i], prompt, seq)
        norm = total / (len(prompt) + L - 1)
        assert abs(norm - scores[i, 0].item()) <= 5e-3, (norm, scores[i, 0].item())
        k = int((lens[i] > 0).sum())
        assert k == beam
        assert all(scores[i, j] >= scores[i, j + 1] - 1e-6 for j in range(k - 1))
        assert margins[i, 0] >= 0 and margins[i, 1] >= 0
        check_engine_margin(margins[i], om[0], eps, f"beam {beam}, sentence {i}")
        if seq != ref[0].seq.tolist():
            step_gap, final_gap = om[0][:2]
            assert oracle_excuses(om[0], eps), (
                f"sentence {i}: tokens differ from the oracle although every decision margin the ORACLE "
                f"measured (step {step_gap:.3e}, final {final_gap:.3e}) is above eps {eps:.3e}; engine's: {margins[i].tolist()}")
            assert abs(norm - ref[0].score) <= 2 * eps, (norm, ref[0].score)
            excused.append((i, step_gap, final_gap))
    print(f"beam {beam}, per-sentence prompts: {N - len(excused)}/{N} best hypotheses token-identical to the oracle; "
          f"excused near-ties (< {eps:.2e}): {len(excused)}: {excused}")
    assert len(excused) <= N // 8, excused


# ------------------------------------------------------------------------------------------ 5. lengths
def test_lengths_follow_each_rows_own_prompt(setup):
    _, ocfg, _, eng = setup
    n = 6
    emb = torch.randn(n, ocfg.model_dim, generator=torch.Generator().manual_seed(5)) * 0.3
    prompts = [[3, 701], [3, 702, 11, 12, 13], [3, 703], [3, 701, 500, 600, 700], [3, 704], [3, 705, 9, 8, 7]]
    toks, lens, _ = eng.generate(emb.cuda(), prompts, beam_size=2, max_gen_len=(0, 4), min_gen_len=2)
    toks, lens = toks.cpu(), lens.cpu()
    assert toks.shape[2] == 5 + 4
    for i in range(n):
        for j in range(2):
            L = int(lens[i, j])
            assert 3 <= L <= 4 and toks[i, j, L - 1].item() == 3   # >= min_gen_len tokens before EOS, <= the row's cap
            assert 3 not in toks[i, j, :L - 1].tolist()
            assert (toks[i, j, L:] == -1).all()
    from sonar_amd.generation import TopKSampler

    toks, lens, _ = eng.sample(emb.cuda(), prompts, TopKSampler(50), max_gen_len=(0, 4), min_gen_len=2, seed=3)
    toks, lens = toks.cpu(), lens.cpu()
    assert toks.shape[1] == 5 + 4
    for i in range(n):
        L = int(lens[i])
        assert 3 <= L <= 4 and toks[i, L - 1].item() == 3 and 3 not in toks[i, :L - 1].tolist()
    full = [[3, 701], [3] + [700] * (ocfg.max_seq_len - 1), [3, 702]]   # row 1: plen + 1 > max_seq_len
    with pytest.raises(ValueError, match="row 1"):
        eng.generate(emb[:3].cuda(), full, beam_size=2)
    with pytest.raises(ValueError, match="row 1"):
        eng.sample(emb[:3].cuda(), full, TopKSampler(5))
    with pytest.raises(ValueError, match="one prompt per sentence"):
        eng.generate(emb.cuda(), prompts[:5], beam_size=2)
    with pytest.raises(ValueError, match="row 2"):   # a token outside the vocabulary: refused by the library, naming the row
        eng.generate(emb[:3].cuda(), [[3, 701], [3, 702], [3, ocfg.vocab_size]], beam_size=2, max_gen_len=(0, 4))


# ------------------------------------------------------------------------------------------ 6. pipeline
def test_pipeline_target_languages_and_prefixes(setup, tmp_path):
    import sentencepiece as spm

    from sonar_amd.inference_pipelines import EmbeddingToTextModelPipeline
    from sonar_amd.text_decoder import ConditionalTransformerDecoderModel
    from sonar_amd.tokenizer import NllbTokenizer

    OD, _, _, _ = setup
    words = ["hello", "world", "my", "name", "is", "paul", "teacher", "working", "bonjour", "monde"]
    corpus = tmp_path / "c.txt"
    g = torch.Generator().manual_seed(0)
    with open(corpus, "w") as fh:
        for _ in range(300):
            n = int(torch.randint(2, 10, (1,), generator=g))
            fh.write(" ".join(words[int(i)] for i in torch.randint(0, len(words), (n,), generator=g)) + "\n")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "toy"), vocab_size=40,
                                   model_type="unigram", hard_vocab_limit=False, bos_id=1, eos_id=2,
                                   unk_id=0, pad_id=-1, minloglevel=2)
    tok = NllbTokenizer(str(tmp_path / "toy.model"))
    ocfg, cfg = _cfgs(vocab=tok.vocab_info.size)
    params = OD.make_synthetic_params(ocfg, seed=77, std=0.09)
    model = ConditionalTransformerDecoderModel(cfg, params, device="cuda:0")
    pipe = EmbeddingToTextModelPipeline(model, tok, device=torch.device("cuda:0"))
    n = 10
    emb = torch.randn(n, ocfg.model_dim, generator=torch.Generator().manual_seed(9)) * 0.3
    langs = ["fra_Latn", "eng_Latn", "deu_Latn", "fra_Latn", "spa_Latn", "spa_Latn", "eng_Latn", "fra_Latn", "deu_Latn",
             "eng_Latn"]
    # random weights like the language tokens as much as the pieces, and the decoder drops those: keep the search on the
    # pieces so that the texts say something
    from sonar_amd.generation import BannedSequenceProcessor

    pieces_only = BannedSequenceProcessor([(t,) for t in range(tok.lang_base, tok.vocab_info.size)] + [(1,), (2,)])
    kw = dict(batch_size=4, max_gen_len=(0, 9), step_processors=[pieces_only])
    got = pipe.predict(emb, target_lang=langs, **kw)
    want = [None] * n
    for b0 in range(0, n, 4):          # the same batches, one language at a time: the same row counts
        rows = list(range(b0, min(b0 + 4, n)))
        for L in dict.fromkeys(langs[i] for i in rows):
            one = pipe.predict(emb[rows], target_lang=L, **kw)
            for k, i in enumerate(rows):
                if langs[i] == L:
                    want[i] = one[k]
    assert got == want
    assert all(got) and len(set(got)) > 1, got
    # forced prefixes: the output begins with the prefix's decoded text
    prefixes = ["hello world", None, "my name", "bonjour", None, "teacher working is", "paul", None, "monde", "hello"]
    out = pipe.predict(emb, target_lang=langs, prefixes=prefixes, **kw)
    assert len(out) == n
    for i, pre in enumerate(prefixes):
        if pre is None:
            assert out[i] == got[i]     # no prefix: the row is the one of the call without prefixes (same batches)
        else:
            assert out[i].startswith(tok.decode(tok.create_encoder(lang=langs[i], mode="target").ids(pre))), (out[i], pre)
    one_lang = pipe.predict(emb, target_lang="fra_Latn", prefixes=prefixes, **kw)
    fra = tok.create_encoder(lang="fra_Latn", mode="target")
    assert all(t.startswith(tok.decode(fra.ids(p))) for t, p in zip(one_lang, prefixes) if p)
    # scoring with one language per input == the per-language score calls
    texts = ["hello world", "my name is paul", "bonjour monde", "teacher", "working", "hello", "monde", "paul is", "name",
             "world hello"]
    s_mixed = pipe.score(emb, texts, target_lang=langs, batch_size=4)
    s_want = torch.zeros(n)
    for L in dict.fromkeys(langs):
        rows = [i for i in range(n) if langs[i] == L]
        s_want[rows] = pipe.score(emb[rows], [texts[i] for i in rows], target_lang=L, batch_size=4)
    # the two routes put a text in different company (buckets by length); a token's log-probability is independent of the
    # company within rtol = atol = 1e-5 (tests/test_gpu_decoder_score.py::test_score_batch_independence), and a score sums
    # fewer than 16 of them
    assert max(len(tok.create_encoder(lang="fra_Latn", mode="target").ids(t)) for t in texts) < 16
    assert torch.allclose(s_mixed, s_want, rtol=1e-5, atol=16 * 1e-5), (s_mixed, s_want)
    with pytest.raises(ValueError):
        pipe.predict(emb, target_lang=langs[:3], **kw)
    with pytest.raises(ValueError):
        pipe.predict(emb, target_lang="fra_Latn", prefixes=["hello"], **kw)
