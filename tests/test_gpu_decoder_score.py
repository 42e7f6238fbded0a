"""Teacher-forced scoring (TextDecoderEngine.score / smi_text_decoder_score) on the MI355X: the oracle's log-softmax, the
engine's own logits() route, beam-search scores, tail and batch independence, long rows, chunking, pipelines, bf16."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_decoder import _cfgs  # noqa: E402


def _ragged(lens, t, vocab, seed, fill=None):
    g = torch.Generator().manual_seed(seed)
    toks = torch.randint(4, vocab, (len(lens), t), generator=g)
    toks[:, 0] = 3
    if fill is not None:
        for i, L in enumerate(lens):
            toks[i, L:] = fill
    return toks


def _oracle_logprobs(OD, params, ocfg, emb, toks, lens):
    """[n, t - 1] oracle log-probabilities (0 past each length) and the logit range of every scored position."""
    n, t = toks.shape
    logits = OD.decoder_logits(params, ocfg, emb.float(), toks[:, :t - 1]).double()
    lp = torch.log_softmax(logits, dim=-1).gather(-1, toks[:, 1:, None]).squeeze(-1)
    rng = logits.amax(-1) - logits.amin(-1)
    mask = torch.arange(t - 1)[None, :] < (torch.as_tensor(lens)[:, None] - 1)
    return torch.where(mask, lp, torch.zeros_like(lp)), rng, mask


def _worst(got, ref, rng, mask):
    err = (got.double() - ref).abs() / rng
    return float(err[mask].max()) if mask.any() else 0.0


@pytest.fixture(scope="module")
def small():
    from oracle import text_decoder as OD
    from sonar_amd.text_decoder import TextDecoderEngine

    ocfg, cfg = _cfgs()
    params = OD.make_synthetic_params(ocfg, seed=4321, std=0.09)
    return OD, ocfg, params, TextDecoderEngine(cfg, params, device="cuda:0")


@pytest.mark.parametrize("emb_dtype", [torch.float32, torch.float16])
def test_score_vs_oracle(small, emb_dtype):
    OD, ocfg, params, eng = small
    lens = [1, 2, 5, 17, 33, ocfg.max_seq_len, ocfg.max_seq_len + 1]
    t = max(lens)
    toks = _ragged(lens, t, ocfg.vocab_size, seed=1)
    emb = (torch.randn(len(lens), ocfg.model_dim, generator=torch.Generator().manual_seed(2)) * 0.3).to(emb_dtype)
    got = eng.score(emb.cuda(), toks.cuda(), torch.tensor(lens)).cpu()
    assert got.shape == (len(lens), t - 1) and got.dtype == torch.float32
    ref, rng, mask = _oracle_logprobs(OD, params, ocfg, emb, toks, lens)
    worst = _worst(got, ref, rng, mask)
    print(f"[score] small fast path, {emb_dtype}: worst |delta| / logit range = {worst:.2e} (bar 3e-2)")
    assert worst <= 3e-2
    assert (got[~mask] == 0).all()
    # the list form gives the same values
    lists = [toks[i, :L].tolist() for i, L in enumerate(lens)]
    assert torch.equal(eng.score(emb.cuda(), lists).cpu(), got)


def test_score_generic_path():
    from oracle import text_decoder as OD
    from sonar_amd.text_decoder import TextDecoderEngine

    ocfg, cfg = _cfgs(d=96, heads=3, ffn=192, vocab=700, max_seq_len=40)
    params = OD.make_synthetic_params(ocfg, seed=11, std=0.09)
    eng = TextDecoderEngine(cfg, params, device="cuda:0", dtype=torch.float32)
    lens = [1, 3, 9, 22, 40, 41]
    toks = _ragged(lens, 41, ocfg.vocab_size, seed=3, fill=-1)
    emb = torch.randn(len(lens), 96, generator=torch.Generator().manual_seed(4)) * 0.3
    got = eng.score(emb.cuda(), toks.cuda(), lens).cpu()
    ref, rng, mask = _oracle_logprobs(OD, params, ocfg, emb, toks.clamp(min=0), lens)
    worst = _worst(got, ref, rng, mask)
    print(f"[score] generic (flex) path d=96 x 3 heads: worst |delta| / logit range = {worst:.2e} (bar 1e-4)")
    assert worst <= 1e-4


@pytest.fixture(scope="module")
def basic():
    from sonar_amd.text_decoder import TextDecoderEngine, get_text_decoder_config

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import synth

    cfg = get_text_decoder_config("basic")
    sd = synth.text_decoder_state_dict("cuda:0")
    return cfg, TextDecoderEngine(cfg, sd, device="cuda:0", dtype=torch.float16)


def test_score_vs_logits_route_basic(basic):
    cfg, eng = basic
    V = cfg.vocab_info.size
    lens = [101, 97, 88, 100]
    toks = _ragged(lens, 101, V, seed=5, fill=0)
    emb = torch.randn(4, cfg.model_dim, generator=torch.Generator().manual_seed(6)).half()
    got = eng.score(emb.cuda(), toks.cuda(), lens).cpu().double()
    logits = eng.logits(emb.cuda(), toks[:, :100].cuda())
    rng = (logits.amax(-1) - logits.amin(-1)).cpu().double()
    ref = torch.log_softmax(logits.double(), dim=-1).gather(-1, toks[:, 1:, None].cuda()).squeeze(-1).cpu()
    del logits
    mask = torch.arange(100)[None, :] < (torch.tensor(lens)[:, None] - 1)
    worst = _worst(got, ref, rng, mask)
    print(f"[score] basic fp16 vs logits() + log_softmax: worst |delta| / logit range = {worst:.2e} (bar 5e-3)")
    assert worst <= 5e-3


def test_score_tail_independence_and_bad_ids(small):
    OD, ocfg, params, eng = small
    lens = [4, 9, 1, 30, 12]
    toks = _ragged(lens, 30, ocfg.vocab_size, seed=7)
    emb = torch.randn(5, ocfg.model_dim, generator=torch.Generator().manual_seed(8)).cuda() * 0.3
    base = eng.score(emb, toks.cuda(), lens).cpu()
    g = torch.Generator().manual_seed(9)
    for fill in (-1, ocfg.vocab_size + 7, "random"):
        t2 = toks.clone()
        for i, L in enumerate(lens):
            t2[i, L:] = torch.randint(-50, 2 * ocfg.vocab_size, (30 - L,), generator=g) if fill == "random" else fill
        assert torch.equal(eng.score(emb, t2.cuda(), lens).cpu(), base), fill
    bad = toks.clone()
    bad[1, 8] = ocfg.vocab_size       # the last token of a length-9 row: a target only
    with pytest.raises(ValueError):
        eng.score(emb, bad.cuda(), lens)
    bad = toks.clone()
    bad[3, 5] = -3
    with pytest.raises(ValueError):
        eng.score(emb, bad.cuda(), lens)
    assert torch.equal(eng.score(emb, toks.cuda(), lens).cpu(), base)
    with pytest.raises(ValueError):
        eng.score(emb, toks.cuda(), [4, 9, 0, 30, 12])
    with pytest.raises(ValueError):
        eng.score(emb[:4], toks.cuda(), lens)


def test_score_batch_independence(small):
    OD, ocfg, params, eng = small
    emb = torch.randn(9, ocfg.model_dim, generator=torch.Generator().manual_seed(10)).cuda() * 0.3
    toks = _ragged([20] * 9, 50, ocfg.vocab_size, seed=11)
    alone = eng.score(emb[:1], toks[:1, :20].cuda()).cpu()[0]
    lens = [20, 50, 7, 33, 50, 2, 41, 19, 50]
    company = eng.score(emb, toks.cuda(), lens).cpu()[0, :19]
    wider = torch.zeros(1, 65, dtype=torch.int64)
    wider[0, :20] = toks[0, :20]
    other_t = eng.score(emb[:1], wider.cuda(), [20]).cpu()[0, :19]
    for other in (company, other_t):
        assert torch.allclose(other, alone, rtol=1e-5, atol=1e-5), (other - alone).abs().max()
    print(f"[score] batch independence: in company bit-identical {torch.equal(company, alone)}, "
          f"at another T bit-identical {torch.equal(other_t, alone)}; max |delta| "
          f"{max(float((company - alone).abs().max()), float((other_t - alone).abs().max())):.2e}")


def test_score_matches_beam_search(small):
    OD, ocfg, params, eng = small
    eng.set_beam_logits_dtype(torch.float32)
    eng.set_slab_dtype(torch.float32)
    try:
        emb = torch.randn(3, ocfg.model_dim, generator=torch.Generator().manual_seed(12)).cuda() * 0.3
        prompt = [3, 701]
        capped = 0
        for beam, mgl in ((1, (0, 6)), (5, (0, 6)), (5, (0, 200))):
            toks, lens, scores = eng.generate(emb, prompt, beam_size=beam, max_gen_len=mgl, normalize_scores=False)
            toks, lens, scores = toks.cpu(), lens.cpu(), scores.cpu()
            seqs, owners, want = [], [], []
            for i in range(3):
                for b in range(beam):
                    L = int(lens[i, b])
                    seqs.append(prompt + toks[i, b, :L].tolist())
                    owners.append(i)
                    want.append(float(scores[i, b]))
                    capped += len(seqs[-1]) == toks.shape[2]     # ran to the length cap (forced EOS)
            lp = eng.score(emb[owners], seqs).cpu().double()
            t = lp.shape[1] + 1
            padded = torch.zeros(len(seqs), t, dtype=torch.int64)
            for k, s in enumerate(seqs):
                padded[k, :len(s)] = torch.tensor(s)
            logits = eng.logits(emb[owners], padded[:, :t - 1].cuda())
            rng = float((logits.amax(-1) - logits.amin(-1)).max())
            del logits
            for k, s in enumerate(seqs):
                got = float(lp[k].sum())
                bar = (len(s) - 1) * 5e-3 * rng
                assert abs(got - want[k]) <= bar, (beam, k, got, want[k], bar)
        assert capped >= 1
    finally:
        eng.set_beam_logits_dtype(torch.float16)
        eng.set_slab_dtype(torch.float16)


def test_score_long_rows():
    from oracle import text_decoder as OD
    from sonar_amd.text_decoder import TextDecoderEngine

    ocfg, cfg = _cfgs(max_seq_len=300)
    params = OD.make_synthetic_params(ocfg, seed=13, std=0.09)
    eng = TextDecoderEngine(cfg, params, device="cuda:0")
    lens = [300, 257, 129, 128, 5]
    toks = _ragged(lens, 300, ocfg.vocab_size, seed=14, fill=0)
    emb = torch.randn(5, ocfg.model_dim, generator=torch.Generator().manual_seed(15)) * 0.3
    got = eng.score(emb.cuda(), toks.cuda(), lens).cpu()
    ref, rng, mask = _oracle_logprobs(OD, params, ocfg, emb, toks, lens)
    worst = _worst(got, ref, rng, mask)
    print(f"[score] T = 300: worst |delta| / logit range = {worst:.2e} (bar 3e-2)")
    assert worst <= 3e-2


def test_score_chunking_basic(basic):
    cfg, eng = basic
    V = cfg.vocab_info.size
    g = torch.Generator().manual_seed(16)
    lens = torch.randint(2, 65, (512,), generator=g)
    lens[0] = 64
    toks = _ragged(lens.tolist(), 64, V, seed=17, fill=0).cuda()
    emb = (torch.randn(512, cfg.model_dim, generator=g) * 0.3).half().cuda()
    big = eng.score(emb, toks, lens).cpu()     # 512 x 63 rows: two sentence groups, ten logits chunks each
    parts = []
    for s0 in range(0, 512, 64):
        sl = lens[s0:s0 + 64]
        t = int(sl.max())
        part = torch.zeros(64, 63)
        part[:, :t - 1] = eng.score(emb[s0:s0 + 64], toks[s0:s0 + 64, :t].contiguous(), sl).cpu()
        parts.append(part)
    small_calls = torch.cat(parts)
    d = (big - small_calls).abs().max()
    print(f"[score] 512 x 64 in one call vs 8 calls: max |delta| {float(d):.2e}, bit-identical {torch.equal(big, small_calls)}")
    assert torch.allclose(big, small_calls, rtol=1e-5, atol=1e-5)


def test_score_pipelines(small, tmp_path):
    import sentencepiece as spm

    from oracle import text_encoder as OE
    from sonar_amd.inference_pipelines import EmbeddingToTextModelPipeline, TextToTextModelPipeline
    from sonar_amd.inference_pipelines.text import score_sequences
    from sonar_amd.text_decoder import ConditionalTransformerDecoderModel
    from sonar_amd.text_encoder import SonarTextEncoderConfig, SonarTextTransformerEncoderModel, VocabularyInfo
    from sonar_amd.tokenizer import NllbTokenizer

    OD = small[0]
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
    v = tok.vocab_info.size
    ocfg, cfg = _cfgs(vocab=v)
    params = OD.make_synthetic_params(ocfg, seed=77, std=0.09)
    dec = ConditionalTransformerDecoderModel(cfg, params, device="cuda:0")
    pipe = EmbeddingToTextModelPipeline(dec, tok, device=torch.device("cuda:0"))
    texts = ["hello world my name is paul", "", "bonjour", "teacher working monde monde hello", "is my"]
    emb = torch.randn(5, ocfg.model_dim, generator=torch.Generator().manual_seed(18)) * 0.3
    got = pipe.score(emb, texts, target_lang="fra_Latn", batch_size=2)
    assert got.shape == (5,) and got.dtype == torch.float32 and got.device.type == "cpu"
    seqs, plen = score_sequences(tok, texts, "fra_Latn")
    for i, s in enumerate(seqs):
        st = torch.tensor([s])
        logits = OD.decoder_logits(params, ocfg, emb[i:i + 1], st[:, :-1]).double()
        lp = torch.log_softmax(logits, -1).gather(-1, st[:, 1:, None]).squeeze(-1)[0]
        ref = float(lp[plen - 1:].sum())
        bar = 3e-2 * float((logits.amax(-1) - logits.amin(-1)).max()) * (len(s) - plen)
        assert abs(float(got[i]) - ref) <= bar, (i, float(got[i]), ref, bar)
    # input order is kept and the bucketing does not change the result
    for bs in (1, 5, 64):
        assert torch.allclose(pipe.score(emb, texts, target_lang="fra_Latn", batch_size=bs), got, rtol=1e-5, atol=1e-5)
    # the empty text scores its EOS alone
    eos_only = dec.engine.score(emb[1:2].cuda(), [seqs[1]]).cpu()
    assert seqs[1] == seqs[1][:plen] + [tok.vocab_info.eos_idx]
    assert abs(float(got[1]) - float(eos_only[0, plen - 1])) <= 1e-6

    ecfg = SonarTextEncoderConfig(model_dim=256, num_encoder_layers=2, num_encoder_attn_heads=4, ffn_inner_dim=512,
                                  vocab_info=VocabularyInfo(size=v), _from_fairseq=True)
    eparams = OE.make_synthetic_params(OE.OracleTextEncoderConfig(model_dim=256, num_layers=2, num_heads=4,
                                                                  ffn_inner_dim=512, vocab_size=v), seed=19, std=0.08)
    enc = SonarTextTransformerEncoderModel(ecfg, eparams, device="cuda:0", dtype=torch.float16)
    t2t = TextToTextModelPipeline(enc, dec, tok, device=torch.device("cuda:0"))
    sources = ["hello world", "my name is paul", "bonjour monde"]
    targets = ["bonjour monde", "", "teacher"]
    both = t2t.score(sources, targets, source_lang="eng_Latn", target_lang="fra_Latn", batch_size=2)
    vecs = t2t.t2vec.predict(sources, source_lang="eng_Latn", batch_size=2)
    want = pipe.score(vecs, targets, target_lang="fra_Latn", batch_size=2)
    assert torch.allclose(both, want, rtol=1e-5, atol=1e-5)


def test_score_bf16_model():
    from oracle import text_decoder as OD
    from sonar_amd.text_decoder import TextDecoderEngine

    ocfg, cfg = _cfgs()
    params = {k: v.bfloat16() for k, v in OD.make_synthetic_params(ocfg, seed=20, std=0.09).items()}
    eng = TextDecoderEngine(cfg, params, device="cuda:0", dtype=torch.bfloat16)
    lens = [3, 30, 64, 65]
    toks = _ragged(lens, 65, ocfg.vocab_size, seed=21, fill=0)
    emb = (torch.randn(4, ocfg.model_dim, generator=torch.Generator().manual_seed(22)) * 0.3).bfloat16()
    got = eng.score(emb.cuda(), toks.cuda(), lens).cpu()
    ref, rng, mask = _oracle_logprobs(OD, {k: v.float() for k, v in params.items()}, ocfg, emb.float(), toks, lens)
    worst = _worst(got, ref, rng, mask)
    print(f"[score] bf16 model: worst |delta| / logit range = {worst:.2e} (bar 3e-2)")
    assert worst <= 3e-2
