"""GPU: step processors (n-gram repeat blocking, banned sequences) inside the on-device token selection -- the selection
kernel against torch's masked top-k, and beam search / sampling against the CPU restatement (tests/step_processors_ref.py)."""
import ctypes as C

import pytest
import torch

from tests.step_processors_ref import bans, beam_search_with_bans, rescore

pytestmark = pytest.mark.gpu

EPS_REL = 1e-3
INT_MAX = 0x7FFFFFFF


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


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


# ----------------------------------------------------------------------------------- selection kernel
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


def _select(lib, logits, vocab, k2, hist, f16_tm, pad_idx=0, ngram=1, banned=()):
    from sonar_amd import _lib

    rows, ldl = logits.shape
    lg = logits.clone()
    lg[:, vocab:] = -torch.inf
    t = lg.view(rows, ldl // 256, 256)
    tmax = t.max(dim=2).values
    tsum = torch.where(torch.isfinite(t), torch.exp(t - tmax[:, :, None]), torch.zeros_like(t)).sum(dim=2)
    tile_max, tile_sum = tmax.t().contiguous(), tsum.t().contiguous()
    src = _to_tile_major(logits.half()) if f16_tm else logits.contiguous()
    pval = torch.empty((rows, 16), dtype=torch.float32, device="cuda")
    pidx = torch.empty((rows, 16), dtype=torch.int32, device="cuda")
    pmax = torch.empty(rows, dtype=torch.float32, device="cuda")
    psum = torch.empty(rows, dtype=torch.float32, device="cuda")
    sp, keep = _lib.step_processors_struct(ngram, banned)
    _lib.check(lib.smi_vocab_select_banned(src.data_ptr(), ldl, 1 if f16_tm else 0, rows, vocab, tile_max.data_ptr(),
                                           tile_sum.data_ptr(), k2, pad_idx, hist.data_ptr(), hist.shape[1],
                                           hist.shape[1], C.byref(sp), pval.data_ptr(), pidx.data_ptr(),
                                           pmax.data_ptr(), psum.data_ptr(), _stream()))
    torch.cuda.synchronize()
    del keep
    return pval.cpu(), pidx.cpu(), pmax.cpu(), psum.cpu()


def _adversarial(vocab, rows, L, k2, seed):
    """logits fp32 [rows, ldl] (fp16-exact values) and per-row ban lists realised through n = 1 (a row's history is the
    list of ids it bans, repeated to length L)."""
    g = torch.Generator().manual_seed(seed)
    ldl = (vocab + 255) // 256 * 256
    lg = (torch.randn(rows, ldl, generator=g) * 3).half().float()
    ntiles = (vocab + 255) // 256
    banlists = []
    for r in range(rows):
        kind = r % 7
        row = lg[r, :vocab]
        if kind == 0:     # the row maximum
            ids = [int(row.argmax())]
        elif kind == 1:   # the maxima of the top 24 tiles: more dirty tiles than register slots
            tm = row.new_full((ntiles * 256,), -torch.inf)
            tm[:vocab] = row
            tmax, targ = tm.view(ntiles, 256).max(dim=1)
            top = tmax.argsort(descending=True)[:min(24, ntiles)]
            ids = [int(t) * 256 + int(targ[t]) for t in top]
        elif kind == 2:   # several bans in the best tile
            t = int(row.argmax()) // 256
            seg = row[t * 256:min(vocab, t * 256 + 256)]
            ids = [t * 256 + int(i) for i in seg.argsort(descending=True)[:6]]
        elif kind == 3:   # tile 0: make it hold the largest values, then ban some of them
            lg[r, 1:9] = 40.0 + torch.arange(8).float()
            ids = [2, 5, 8, int(lg[r, :vocab].argmax())]
        elif kind == 4:   # value ties across a dirty and a clean tile
            t1, t2 = min(3, ntiles - 1), min(1, ntiles - 1)
            lg[r, t1 * 256 + 7] = 50.0
            lg[r, t2 * 256 + 200] = 50.0
            lg[r, t1 * 256 + 9] = 51.0
            ids = [t1 * 256 + 9]
        elif kind == 5 and vocab <= L + k2:   # all but < k2 tokens banned
            keep = set(torch.randperm(vocab, generator=g)[:max(k2 - 2, 0)].tolist())
            ids = [i for i in range(vocab) if i not in keep]
        else:             # random bans + the argmax
            ids = torch.randint(0, vocab, (40,), generator=g).tolist() + [int(row.argmax())]
        ids = ids[:L]
        banlists.append(ids)
    hist = torch.tensor([(ids * ((L + len(ids) - 1) // len(ids)))[:L] for ids in banlists], dtype=torch.int32)
    return lg, hist, banlists


def _expected(lg, vocab, banlists, k2, pad_idx=0):
    m = lg[:, :vocab].clone()
    m[:, pad_idx] = -torch.inf
    for r, ids in enumerate(banlists):
        m[r, ids] = -torch.inf
    vals, idx = torch.sort(-m, dim=1, stable=True)   # value desc, token asc
    vals, idx = -vals[:, :k2], idx[:, :k2].int()
    idx[~torch.isfinite(vals)] = INT_MAX
    return vals, idx


# vocab 1000 is 4 tiles, fewer than any k2 > 3: the tile rounds end early, and an odd k2 leaves the arg-max's double buffer on
# either parity when they do; 16 is the largest k2 (VS_K2MAX); k2 = 1 leaves the "all but < k2" row with no candidate at all.
@pytest.mark.parametrize("vocab,k2", [pytest.param(1000, 10, id="1000"), pytest.param(256206, 10, id="256206"),
                                      pytest.param(1000, 1, id="1000-k2_1"), pytest.param(1000, 7, id="1000-k2_7"),
                                      pytest.param(1000, 16, id="1000-k2_16"), pytest.param(256206, 16, id="256206-k2_16")])
@pytest.mark.parametrize("f16_tm", [0, 1])
def test_banned_selection_equals_masked_topk(vocab, k2, f16_tm):
    from sonar_amd import _lib

    lib = _lib.load()
    rows, L = 256, 1000 if vocab == 1000 else 64
    lg, hist, banlists = _adversarial(vocab, rows, L, k2, seed=vocab + f16_tm)
    for r, ids in enumerate(banlists):
        assert set(hist[r].tolist()) == set(ids)
    pval, pidx, pmax, psum = _select(lib, lg.cuda(), vocab, k2, hist.cuda(), f16_tm)
    ev, ei = _expected(lg, vocab, banlists, k2)
    assert torch.equal(pidx[:, :k2], ei), (pidx[:, :k2] != ei).nonzero()[:5]
    assert torch.equal(pval[:, :k2], ev)
    # the normaliser is the untouched row's, bit for bit: with no processor the entry point runs the engine's default
    # selection kernel (vocab_select_kernel), so this compares the banned kernel with the default path
    _, _, pmax0, psum0 = _select(lib, lg.cuda(), vocab, k2, hist.cuda(), f16_tm, ngram=0)
    assert torch.equal(pmax, pmax0) and torch.equal(psum, psum0)
    ref_max = lg[:, :vocab].max(dim=1).values
    assert torch.equal(pmax, ref_max)
    ref_sum = torch.exp(lg[:, :vocab] - ref_max[:, None]).sum(dim=1)
    assert torch.allclose(psum, ref_sum, rtol=1e-4)
    # with no ban at all it is the plain top-k2
    pv0, pi0, _, _ = _select(lib, lg.cuda(), vocab, k2, hist.cuda(), f16_tm, ngram=0)
    ev0, ei0 = _expected(lg, vocab, [[0]] * rows, k2)
    assert torch.equal(pi0[:, :k2], ei0) and torch.equal(pv0[:, :k2], ev0)


def test_banned_selection_banned_sequences():
    from sonar_amd import _lib

    lib = _lib.load()
    vocab, rows, k2, L = 1000, 256, 10, 12
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(rows, 1024, generator=g)
    hist = torch.randint(4, 30, (rows, L), generator=g, dtype=torch.int32)
    banned = [[int(lg[0].argmax())], [5, 6, 7]] + [hist[r, -2:].tolist() + [int(lg[r, :vocab].argmax())] for r in range(0, 40)]
    pval, pidx, _, _ = _select(lib, lg.cuda(), vocab, k2, hist.cuda(), 0, ngram=2, banned=banned)
    lists = [sorted(bans(hist[r].tolist(), 2, banned)) or [0] for r in range(rows)]
    ev, ei = _expected(lg, vocab, lists, k2)
    assert torch.equal(pidx[:, :k2], ei) and torch.equal(pval[:, :k2], ev)
    assert sum(len(x) > 1 for x in lists) >= 30


def test_set_step_processors_validates(setup):
    from sonar_amd import _lib

    _, _, _, eng = setup
    bad = [(0, [[5000]]), (65, []), (-1, []), (0, [[1], []])]
    for n, seqs in bad:
        sp, keep = _lib.step_processors_struct(n, seqs)
        assert eng.lib.smi_text_decoder_set_step_processors(eng._handle, C.byref(sp)) != 0, (n, seqs)
    assert eng.lib.smi_text_decoder_set_step_processors(eng._handle, None) == 0


# ----------------------------------------------------------------------------------- beam search
def _check_hyps(OD, params, ocfg, emb, prompt, toks, lens, scores, n_gram, banned, max_len, score_tol=5e-3):
    """every hypothesis: no ban violated on its free steps, score = the oracle's rescoring of its tokens."""
    n, beam = lens.shape
    for i in range(n):
        for j in range(beam):
            L = int(lens[i, j])
            if L == 0:
                continue
            seq = toks[i, j, :L].tolist()
            full = list(prompt) + seq
            for p in range(len(prompt), len(full)):
                if p == max_len - 1:      # the forced EOS at the length cap
                    continue
                assert full[p] not in bans(full[:p], n_gram, banned), (i, j, p, full)
            lp = rescore(OD, params, ocfg, emb[i], prompt, seq)
            # the prompt's forced tokens count in the length and the sum (oracle/beam_search_incremental)
            pre = rescore(OD, params, ocfg, emb[i], prompt[:1], prompt[1:]).sum().item() if len(prompt) > 1 else 0.0
            norm = (lp.sum().item() + pre) / (len(prompt) + L - 1)
            assert abs(norm - scores[i, j].item()) <= score_tol, (i, j, norm, scores[i, j].item())


@pytest.mark.parametrize("n_gram", [2, 3])
def test_greedy_validity_under_blocking(setup, n_gram):
    """beam 1: at every free step the engine's token is unbanned and within EPS_REL x the logit range of the masked oracle
    maximum, re-scored on the engine's own prefix (robust to near-ties, which whole-sequence parity is not here)."""
    from sonar_amd.generation import NGramRepeatBlockProcessor

    OD, ocfg, params, eng = setup
    n, prompt = 12, [3, 7]
    emb = torch.randn(n, ocfg.model_dim, generator=torch.Generator().manual_seed(40 + n_gram)) * 0.3
    toks, lens, _ = eng.generate(emb.cuda(), prompt, beam_size=1, max_gen_len=(0, 30),
                                 step_processors=[NGramRepeatBlockProcessor(n_gram)])
    toks, lens = toks.cpu(), lens.cpu()
    max_len = len(prompt) + 30
    checked = 0
    for i in range(n):
        seq = toks[i, 0, :int(lens[i, 0])].tolist()
        full = prompt + seq
        lg = OD.decoder_logits(params, ocfg, emb[i:i + 1], torch.tensor([full[:-1]]))[0]
        eps = EPS_REL * (lg.max() - lg.min()).item()
        for p in range(len(prompt), len(full)):
            if p == max_len - 1:
                continue
            row = lg[p - 1].clone()
            row[0] = -torch.inf
            if p < len(prompt) + 1:
                row[3] = -torch.inf
            banned = bans(full[:p], n_gram)
            assert full[p] not in banned, (i, p, full)
            if banned:
                row[sorted(banned)] = -torch.inf
            assert row[full[p]] >= row.max() - eps, (i, p, row[full[p]].item(), row.max().item())
            checked += 1
    assert checked >= n * 5


def _beam_case(OD, ocfg, params, eng, n_gram, banned, seed, n=8, max_new=24, chains=None):
    from sonar_amd.generation import BannedSequenceProcessor, NGramRepeatBlockProcessor
    from tests.neartie import check_engine_margin, oracle_excuses

    prompt = [3, 7]
    emb = torch.randn(n, ocfg.model_dim, generator=torch.Generator().manual_seed(seed)) * 0.3
    procs = ([NGramRepeatBlockProcessor(n_gram)] if n_gram else []) + ([BannedSequenceProcessor(banned)] if banned else [])
    kw = dict(beam_size=5, max_gen_len=(0, max_new))
    toks, lens, scores = eng.generate(emb.cuda(), prompt, step_processors=procs, **kw)
    margins = eng.last_margins(n).cpu()
    toks, lens, scores = toks.cpu(), lens.cpu(), scores.cpu()
    _check_hyps(OD, params, ocfg, emb, prompt, toks, lens, scores, n_gram, banned, len(prompt) + max_new)
    om = []
    ref = beam_search_with_bans(params, ocfg, emb, prompt, margins_out=om, ngram=n_gram, banned_seqs=banned, **kw)
    lg = OD.decoder_logits(params, ocfg, emb, torch.tensor([prompt] * n))
    eps = EPS_REL * (lg.max() - lg.min()).item()
    excused = 0
    for i in range(n):
        seq = toks[i, 0, :int(lens[i, 0])].tolist()
        check_engine_margin(margins[i], om[i], eps, f"n-gram {n_gram}, sentence {i}")
        if seq != ref[i][0].seq.tolist():
            assert oracle_excuses(om[i], eps), (i, seq, ref[i][0].seq.tolist(), om[i])
            excused += 1
    assert excused <= max(1, n // 4), excused
    return toks, lens, scores


@pytest.mark.parametrize("n_gram", [1, 2, 3])
def test_beam5_blocking_mfma(setup, n_gram):
    OD, ocfg, params, eng = setup
    _beam_case(OD, ocfg, params, eng, n_gram, [[11], [7, 500], [3, 7, 900]], seed=60 + n_gram)


@pytest.mark.parametrize("n_gram", [1, 2, 3])
def test_beam5_blocking_flex(toy, n_gram):
    OD, ocfg, params, eng = toy
    _beam_case(OD, ocfg, params, eng, n_gram, [[12], [7, 100]], seed=70 + n_gram, n=6, max_new=16)


def test_blocking_changes_the_output(setup):
    """the repository's own looping decoder: without blocking the best hypotheses repeat, with n = 2 they do not."""
    from sonar_amd.generation import NGramRepeatBlockProcessor

    OD, ocfg, params, eng = setup
    emb = (torch.randn(6, ocfg.model_dim, generator=torch.Generator().manual_seed(1)) * 0.3).cuda()
    plain = eng.generate(emb, [3, 7], max_gen_len=(0, 40))[0].cpu()
    blocked = eng.generate(emb, [3, 7], max_gen_len=(0, 40), step_processors=[NGramRepeatBlockProcessor(2)])[0].cpu()
    assert not torch.equal(plain, blocked)


def test_chains_and_fp16_logits_under_bans(setup):
    from sonar_amd.generation import NGramRepeatBlockProcessor

    OD, ocfg, params, eng = setup
    n = 160   # 800 rows: two chains of >= 384 rows
    emb = (torch.randn(n, ocfg.model_dim, generator=torch.Generator().manual_seed(8)) * 0.3).cuda()
    kw = dict(beam_size=5, max_gen_len=(0, 20), step_processors=[NGramRepeatBlockProcessor(2)])
    from sonar_amd import _lib

    _lib.set_tuning(DEC_KS_OUT=2, DEC_FFN1_ENGINE=1)
    try:
        eng.set_chains(1)
        one = [t.cpu() for t in eng.generate(emb, [3, 7], **kw)]
        eng.set_chains(2)
        two = [t.cpu() for t in eng.generate(emb, [3, 7], **kw)]
    finally:
        eng.set_chains(0)
        _lib.set_tuning(DEC_KS_OUT=None, DEC_FFN1_ENGINE=None)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    # both storage types of the logits (this engine's default is float16)
    for dt in (torch.float16, torch.float32):
        eng.set_beam_logits_dtype(dt)
        try:
            toks, lens, scores = eng.generate(emb[:8], [3, 7], **kw)
        finally:
            eng.set_beam_logits_dtype(torch.float16)
        _check_hyps(OD, params, ocfg, emb[:8].cpu(), [3, 7], toks.cpu(), lens.cpu(), scores.cpu(), 2, (), 22)


def test_default_path_unchanged(setup):
    from sonar_amd.generation import NGramRepeatBlockProcessor

    OD, ocfg, params, eng = setup
    emb = (torch.randn(10, ocfg.model_dim, generator=torch.Generator().manual_seed(2)) * 0.3).cuda()
    a = [t.cpu() for t in eng.generate(emb, [3, 7], max_gen_len=(0, 20))]
    eng.generate(emb, [3, 7], max_gen_len=(0, 20), step_processors=[NGramRepeatBlockProcessor(1)])
    eng.set_step_processors(None)
    b = [t.cpu() for t in eng.generate(emb, [3, 7], max_gen_len=(0, 20))]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------------- sampling
def test_sampling_under_bans(setup):
    from sonar_amd.generation import BannedSequenceProcessor, NGramRepeatBlockProcessor, TopKSampler, TopPSampler

    OD, ocfg, params, eng = setup
    n, prompt = 12, [3, 7]
    emb = (torch.randn(n, ocfg.model_dim, generator=torch.Generator().manual_seed(5)) * 0.3).cuda()
    procs = [NGramRepeatBlockProcessor(2)]
    # top-1 sampling under blocking is the greedy search under the same blocking
    # (fp32 logits on both sides: the sampler reads fp32 rows, and fp16 storage would tie what fp32 separates)
    st, sl, _ = eng.sample(emb, prompt, TopKSampler(1), max_gen_len=(0, 24), seed=1, step_processors=procs)
    eng.set_beam_logits_dtype(torch.float32)
    try:
        bt, bl, _ = eng.generate(emb, prompt, beam_size=1, max_gen_len=(0, 24), step_processors=procs)
    finally:
        eng.set_beam_logits_dtype(torch.float16)
    st, sl, bt, bl = st.cpu(), sl.cpu(), bt.cpu(), bl.cpu()
    for i in range(n):
        L = int(sl[i])
        assert L == int(bl[i, 0]) and st[i, :L].tolist() == bt[i, 0, :L].tolist(), i
    # nucleus sampling: never a banned token on a free step, and a fixed seed repeats
    procs = [NGramRepeatBlockProcessor(1), BannedSequenceProcessor([[20], [3, 7, 30]])]
    t1, l1, s1 = [x.cpu() for x in eng.sample(emb, prompt, TopPSampler(0.95), max_gen_len=(0, 16), seed=9,
                                               step_processors=procs)]
    t2, l2, s2 = [x.cpu() for x in eng.sample(emb, prompt, TopPSampler(0.95), max_gen_len=(0, 16), seed=9,
                                               step_processors=procs)]
    assert torch.equal(t1, t2) and torch.equal(l1, l2) and torch.equal(s1, s2)
    max_len = len(prompt) + 16
    for i in range(n):
        full = prompt + t1[i, :int(l1[i])].tolist()
        for p in range(len(prompt), len(full)):
            if p != max_len - 1:
                assert full[p] not in bans(full[:p], 1, [[20], [3, 7, 30]]), (i, p, full)
    # n = 1 bans the prompt's </s>: every sentence runs to the length cap
    assert (l1 == 16).all()


# ----------------------------------------------------------------------------------- pipelines
def test_pipelines_accept_step_processors(setup, tmp_path):
    import sentencepiece as spm

    from sonar_amd.generation import NGramRepeatBlockProcessor, TopKSampler
    from sonar_amd.inference_pipelines import EmbeddingToTextModelPipeline
    from sonar_amd.text_decoder import ConditionalTransformerDecoderModel
    from sonar_amd.tokenizer import NllbTokenizer

    OD, _, _, _ = setup
    words = ["hello", "world", "my", "name", "is", "paul", "teacher", "working", "bonjour", "monde"]
    corpus = tmp_path / "c.txt"
    g = torch.Generator().manual_seed(0)
    with open(corpus, "w") as fh:
        for _ in range(300):
            k = int(torch.randint(2, 10, (1,), generator=g))
            fh.write(" ".join(words[int(i)] for i in torch.randint(0, len(words), (k,), generator=g)) + "\n")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "toy"), vocab_size=40,
                                   model_type="unigram", hard_vocab_limit=False, bos_id=1, eos_id=2,
                                   unk_id=0, pad_id=-1, minloglevel=2)
    tok = NllbTokenizer(str(tmp_path / "toy.model"))
    ocfg, cfg = _cfgs(vocab=tok.vocab_info.size)
    params = OD.make_synthetic_params(ocfg, seed=77, std=0.09)
    model = ConditionalTransformerDecoderModel(cfg, params, device="cuda:0")
    pipe = EmbeddingToTextModelPipeline(model, tok, device=torch.device("cuda:0"))
    emb = torch.randn(4, ocfg.model_dim, generator=torch.Generator().manual_seed(9)) * 0.3
    look = type("NGramRepeatBlockProcessor", (), {"ngram_size": 2})()
    ours = pipe.predict(emb, target_lang="fra_Latn", max_gen_len=(0, 9), step_processors=[NGramRepeatBlockProcessor(2)])
    theirs = pipe.predict(emb, target_lang="fra_Latn", max_gen_len=(0, 9), step_processors=[look])
    assert ours == theirs and len(ours) == 4
    sampled = pipe.predict(emb, target_lang="fra_Latn", max_gen_len=(0, 9), sampler=TopKSampler(1),
                           step_processors=[look])
    assert len(sampled) == 4 and all(isinstance(t, str) for t in sampled)
    with pytest.raises(NotImplementedError):
        pipe.predict(emb, target_lang="fra_Latn", step_processors=[object()])
    # the handle is cleared after a call: the default path runs again
    assert pipe.predict(emb, target_lang="fra_Latn", max_gen_len=(0, 9)) == \
        pipe.predict(emb, target_lang="fra_Latn", max_gen_len=(0, 9), step_processors=[])


# ----------------------------------------------------------------------------------- one sampling step under bans
SAMPLE_BANNED = (3, 7, 9, 11, 12, 500)   # hist [3, 7, 500, 9] under n = 1, plus the sequences [11] and [9, 12]


def _sample_rows_banned(logits, sampler, z, temperature=1.0):
    from sonar_amd import _lib

    lib = _lib.load()
    rows, v = logits.shape
    ld = (v + 255) // 256 * 256
    buf = torch.full((rows, ld), 7.5, dtype=torch.float32, device="cuda")
    buf[:, :v] = logits.cuda()
    zt = torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in z], dtype=torch.int64, device="cuda")
    hist = torch.tensor([3, 7, 500, 9], dtype=torch.int32, device="cuda")
    tok = torch.empty(rows, dtype=torch.int32, device="cuda")
    lp = torch.empty(rows, dtype=torch.float32, device="cuda")
    mass = torch.empty(rows, dtype=torch.int64, device="cuda")
    cnt = torch.empty(rows, dtype=torch.int32, device="cuda")
    kind = _lib.SMI_SAMPLER_TOP_K if sampler[0] == "top_k" else _lib.SMI_SAMPLER_TOP_P
    sp, keep = _lib.step_processors_struct(1, [[11], [9, 12]])
    _lib.check(lib.smi_sample_rows_banned(buf.data_ptr(), ld, rows, v, kind, int(sampler[1]) if kind == 0 else 1,
                                          float(sampler[1]) if kind == 1 else 1.0, temperature, 0, 3, 0, 1, 0.0,
                                          hist.data_ptr(), 4, C.byref(sp), zt.data_ptr(), tok.data_ptr(), lp.data_ptr(),
                                          mass.data_ptr(), cnt.data_ptr(), _stream()))
    torch.cuda.synchronize()
    del keep
    return tok.cpu().tolist(), lp.cpu(), mass.cpu().tolist(), cnt.cpu().tolist()


@pytest.mark.parametrize("sampler", [("top_k", 1), ("top_k", 50), ("top_p", 0.5), ("top_p", 0.9)])
def test_sampling_step_under_bans_vs_q40(sampler):
    """One filter + draw with bans against the CPU Q40 restatement: banned masses 0, Z and M the untouched row's."""
    from oracle import text_decoder as OD

    g = torch.Generator().manual_seed(21)
    rows = 24
    logits = torch.randn(rows, 1000, generator=g) * 3.0
    logits[:, 500] = logits.max(dim=1).values + 1.0      # the loop token: every row's maximum, banned
    z = [OD.splitmix_word(33, r, 5) for r in range(rows)]
    tok, lp, mass, cnt = _sample_rows_banned(logits, sampler, z)
    checked = 0
    for r in range(rows):
        masses, _ = OD.q40_masses(logits[r])
        probs = OD.sampling_probs(logits[r])              # untouched normaliser, PAD zeroed
        probs[list(SAMPLE_BANNED)] = 0.0
        masses[list(SAMPLE_BANNED) + [0]] = 0
        assert tok[r] not in SAMPLE_BANNED and tok[r] != 0, (r, tok[r])
        assert lp[r].item() == pytest.approx(float(torch.log(probs[tok[r]])), abs=2e-4)
        masked = logits[r].clone()
        masked[list(SAMPLE_BANNED) + [0]] = -torch.inf
        if sampler[0] == "top_p":   # the nucleus of the banned probabilities, not renormalised
            sp = torch.sort(probs, descending=True).values.double()
            excl = torch.cumsum(sp, 0) - sp
            npos = int((sp > 0).sum())
            lo = int((excl[:npos] <= sampler[1] - 2e-6).sum())
            hi = int((excl[:npos] <= sampler[1] + 2e-6).sum())
            assert lo <= cnt[r] <= hi, (r, lo, cnt[r], hi)
            keep = OD.sample_filter(masked, ("top_k", cnt[r])).numpy()
        else:
            keep = OD.sample_filter(masked, sampler).numpy()
        assert cnt[r] == int(keep.sum()), (r, cnt[r], int(keep.sum()))
        want_mass = int(masses[keep].astype(object).sum())
        assert abs(mass[r] - want_mass) <= 4e-6 * want_mass + 64
        want_tok, margin = OD.sample_draw(masses, keep, z[r])
        if margin > 2e-6:
            assert tok[r] == want_tok, (r, tok[r], want_tok)
            checked += 1
    assert checked >= rows // 2


@pytest.mark.parametrize("sampler", [("top_k", 5), ("top_p", 0.9)])
def test_sampling_step_with_no_kept_mass(sampler):
    """The banned token holds M far above the rest: every kept Q40 mass is 0.  The most probable kept token comes back
    (lowest id on a tie), with its exact log-probability."""
    g = torch.Generator().manual_seed(22)
    rows = 8
    logits = torch.randn(rows, 1000, generator=g)
    logits[:, 500] = 200.0
    logits[1, 40] = logits[1, 41] = 10.0            # a value tie among the kept: the lower id wins
    tok, lp, mass, _ = _sample_rows_banned(logits, sampler, [0x5555 * (r + 1) for r in range(rows)])
    ref_lp = torch.log_softmax(logits.double(), dim=-1)
    for r in range(rows):
        masked = logits[r].clone()
        masked[list(SAMPLE_BANNED) + [0]] = -torch.inf
        assert mass[r] == 0
        assert tok[r] == int(masked.argmax()), (r, tok[r])
        assert lp[r].item() == pytest.approx(ref_lp[r, tok[r]].item(), abs=1e-3)
    assert tok[1] == 40


def test_sampling_low_temperature_under_blocking(setup):
    """The engine at temperature 0.05 with n = 1: the blocked token dominates every row, and the draw still returns
    valid, unbanned tokens."""
    from sonar_amd.generation import NGramRepeatBlockProcessor, TopKSampler, TopPSampler

    OD, ocfg, params, eng = setup
    n, prompt = 8, [3, 7]
    emb = (torch.randn(n, ocfg.model_dim, generator=torch.Generator().manual_seed(6)) * 0.3).cuda()
    for smp in (TopKSampler(20), TopPSampler(0.9)):
        t, l, s = [x.cpu() for x in eng.sample(emb, prompt, smp, temperature=0.05, max_gen_len=(0, 16), seed=3,
                                                step_processors=[NGramRepeatBlockProcessor(1)])]
        for i in range(n):
            full = prompt + t[i, :int(l[i])].tolist()
            assert all(0 < x < ocfg.vocab_size for x in full[len(prompt):]), full
            for p in range(len(prompt), len(full) - 1):
                assert full[p] not in bans(full[:p], 1), (i, p, full)
            assert torch.isfinite(s[i])


def test_sampling_with_every_token_banned(toy):
    """A small vocabulary can be banned entirely: the row ends with EOS at log-probability -inf."""
    from sonar_amd.generation import BannedSequenceProcessor, TopKSampler

    OD, ocfg, params, eng = toy
    emb = (torch.randn(3, ocfg.model_dim, generator=torch.Generator().manual_seed(7)) * 0.3).cuda()
    every = BannedSequenceProcessor([[t] for t in range(ocfg.vocab_size)])
    t, l, s = [x.cpu() for x in eng.sample(emb, [3, 7], TopKSampler(5), max_gen_len=(0, 8), seed=1,
                                            step_processors=[every])]
    assert (l == 1).all() and (t[:, 0] == 3).all() and torch.isinf(s).all() and (s < 0).all()


# ----------------------------------------------------------------------------------- TextToText
def test_text_to_text_pipeline_with_step_processors(setup, tmp_path):
    import sentencepiece as spm

    from oracle import text_encoder as OE
    from sonar_amd.generation import NGramRepeatBlockProcessor
    from sonar_amd.inference_pipelines import (EmbeddingToTextModelPipeline, TextToEmbeddingModelPipeline,
                                               TextToTextModelPipeline)
    from sonar_amd.text_decoder import ConditionalTransformerDecoderModel
    from sonar_amd.text_encoder import SonarTextEncoderConfig, SonarTextTransformerEncoderModel, VocabularyInfo
    from sonar_amd.tokenizer import NllbTokenizer

    OD, _, _, _ = setup
    words = ["hello", "world", "my", "name", "is", "paul", "teacher", "working", "bonjour", "monde"]
    corpus = tmp_path / "c.txt"
    g = torch.Generator().manual_seed(0)
    with open(corpus, "w") as fh:
        for _ in range(300):
            k = int(torch.randint(2, 10, (1,), generator=g))
            fh.write(" ".join(words[int(i)] for i in torch.randint(0, len(words), (k,), generator=g)) + "\n")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "toy"), vocab_size=40,
                                   model_type="unigram", hard_vocab_limit=False, bos_id=1, eos_id=2,
                                   unk_id=0, pad_id=-1, minloglevel=2)
    tok = NllbTokenizer(str(tmp_path / "toy.model"))
    v = tok.vocab_info.size
    ocfg, cfg = _cfgs(vocab=v)
    dec = ConditionalTransformerDecoderModel(cfg, OD.make_synthetic_params(ocfg, seed=77, std=0.09), device="cuda:0")
    oe = OE.OracleTextEncoderConfig(model_dim=256, num_layers=2, num_heads=4, ffn_inner_dim=512, vocab_size=v)
    ecfg = SonarTextEncoderConfig(model_dim=256, num_encoder_layers=2, num_encoder_attn_heads=4, ffn_inner_dim=512,
                                  vocab_info=VocabularyInfo(size=v), _from_fairseq=True)
    enc = SonarTextTransformerEncoderModel(ecfg, OE.make_synthetic_params(oe, seed=3, std=0.08), device="cuda:0",
                                           dtype=torch.float16)
    dev = torch.device("cuda:0")
    texts = ["hello world", "my name is paul", "bonjour monde"]
    look = type("NGramRepeatBlockProcessor", (), {"ngram_size": 2})()
    t2t = TextToTextModelPipeline(enc, dec, tok, device=dev)
    got = t2t.predict(texts, source_lang="eng_Latn", target_lang="fra_Latn", batch_size=2, max_gen_len=(0, 7),
                      step_processors=[NGramRepeatBlockProcessor(2)])
    emb = TextToEmbeddingModelPipeline(enc, tok, device=dev).predict(texts, source_lang="eng_Latn")
    want = EmbeddingToTextModelPipeline(dec, tok, device=dev).predict(emb, target_lang="fra_Latn", max_gen_len=(0, 7),
                                                                     step_processors=[look])
    assert got == want and len(got) == 3
    with pytest.raises(NotImplementedError):
        t2t.predict(texts, source_lang="eng_Latn", target_lang="fra_Latn", step_processors=[object()])


# ----------------------------------------------------------------------------------- full size
def test_basic_decoder_full_size_under_blocking():
    """text_sonar_basic_decoder (24 layers, d 1024, V 256 206, fp16 model): 2 sentences, beam 5, n = 2, <= 24 new tokens,
    against the CPU restatement: no ban violated, scores = the fp32 oracle's rescoring, token parity under the near-tie
    excuse.  Covers the real logits GEMM's tile statistics under bans."""
    import torch.nn.functional as F

    from oracle import text_decoder as OD
    from sonar_amd.generation import NGramRepeatBlockProcessor
    from sonar_amd.text_decoder import TextDecoderEngine, get_text_decoder_config
    from tests.neartie import oracle_excuses
    from tools.synth import text_decoder_state_dict

    dev = torch.device("cuda:0")
    sd = text_decoder_state_dict(dev)
    eng = TextDecoderEngine(get_text_decoder_config("basic"), sd, device=dev)
    params = {k: v.detach().float().cpu() for k, v in sd.items()}
    del sd
    torch.cuda.empty_cache()
    ocfg = OD.OracleTextDecoderConfig(model_dim=1024, num_layers=24, num_heads=16, ffn_inner_dim=8192,
                                      vocab_size=256206, max_seq_len=512)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    prompt, max_new = [3, 256047], 24
    emb = F.normalize(torch.randn(2, 1024, generator=torch.Generator().manual_seed(12)), dim=-1) * 0.2
    kw = dict(beam_size=5, max_gen_len=(0, max_new))
    toks, lens, scores = [x.cpu() for x in eng.generate(emb.cuda(), prompt, step_processors=[NGramRepeatBlockProcessor(2)],
                                                        **kw)]
    _check_hyps(OD, params, ocfg, emb, prompt, toks, lens, scores, 2, (), len(prompt) + max_new)
    om = []
    ref = beam_search_with_bans(params, ocfg, emb, prompt, margins_out=om, ngram=2, **kw)
    lg = OD.decoder_logits(params, ocfg, emb, torch.tensor([prompt] * 2))
    eps = 5e-3 * lg.abs().max().item()
    for i in range(2):
        seq = toks[i, 0, :int(lens[i, 0])].tolist()
        if seq != ref[i][0].seq.tolist():
            assert oracle_excuses(om[i], eps), (i, seq, ref[i][0].seq.tolist(), om[i])
    del eng
    torch.cuda.empty_cache()
