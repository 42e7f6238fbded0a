"""GPU: the LASER2 BiLSTM encoder (sonar_amd/laser2.py, csrc/laser2.hip) against the reference's LaserLstmEncoder.

Fixtures: tests/golden/laser2_reference.pt holds outputs of the reference's OWN module (make_golden_laser2.py).  The
full-width cases compare with a CPU fp32 nn.LSTM + pack_padded_sequence restatement of laser_lstm_encoder.py:60-116.
Tolerances (per sentence, against fp32): 1 - cos <= 1e-5 and max |delta| <= 5e-3."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "laser2_reference.pt")
DEV = "cuda:0"
COS_TOL, ABS_TOL = 1e-5, 5e-3


def _assert_close(got, ref, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    cos = F.cosine_similarity(got.double(), ref.double(), dim=-1)
    worst_cos = (1 - cos).max().item()
    worst_abs = (got - ref).abs().max().item()
    assert worst_cos <= COS_TOL and worst_abs <= ABS_TOL, (what, worst_cos, worst_abs)
    return worst_cos, worst_abs


def _fixture_state_dict(case):
    return {k: c.float() * case["scale"] for k, c in case["codes"].items()}


def _cfg(case, padding_value=0.0):
    from sonar_amd.laser2 import Laser2Config

    return Laser2Config(padding_value=padding_value, **case["config"])


def test_fixture_cases_match_the_reference_module():
    from sonar_amd.laser2 import Laser2Model

    fx = torch.load(GOLDEN, weights_only=True)
    seen = set()
    for case in fx["cases"]:
        sd = _fixture_state_dict(case)
        models = {}
        for run in case["runs"]:
            pv = run["padding_value"]
            if pv not in models:
                models[pv] = Laser2Model(_cfg(case, pv), sd, device=DEV)
            out = models[pv](run["seqs"], run["seq_lens"])
            _assert_close(out, run["out"], f"{case['name']} {run['batch']} pv={pv}")
            seen.add((case["name"], run["batch"]))
    assert len(seen) == 15


# ---- full width: the laser2 arch with a cut vocabulary against a CPU fp32 restatement ---------------------------------

def _full_cfg(vocab=4000):
    from sonar_amd.laser2 import get_laser2_config

    cfg = get_laser2_config("laser2")
    cfg.vocabulary_size = vocab
    return cfg


def _random_state_dict(cfg, seed=7):
    from sonar_amd.laser2 import _lstm_keys

    g = torch.Generator().manual_seed(seed)
    lim = cfg.hidden_size ** -0.5
    sd = {"embed_tokens.weight": torch.randn(cfg.vocabulary_size, cfg.model_dim, generator=g) * 0.5}
    sd["embed_tokens.weight"][cfg.pad_idx] = 0
    for group in _lstm_keys(cfg):
        for k, shape in group:
            sd[k] = (torch.rand(shape, generator=g) * 2 - 1) * lim
    return sd


def cpu_laser2(cfg, sd, seqs, lens):
    """laser_lstm_encoder.py:60-116 restated with torch's fp32 nn.LSTM on the CPU."""
    nd = 2 if cfg.bidirectional else 1
    emb = torch.nn.Embedding(cfg.vocabulary_size, cfg.model_dim, padding_idx=cfg.pad_idx)
    lstm = torch.nn.LSTM(cfg.model_dim, cfg.hidden_size, cfg.num_layers, bidirectional=cfg.bidirectional)
    with torch.no_grad():
        emb.weight.copy_(sd["embed_tokens.weight"])
        for k, v in sd.items():
            if k.startswith("lstm."):
                getattr(lstm, k[5:]).copy_(v)
    lens = torch.as_tensor(lens).long()
    order = torch.argsort(-lens)
    x, l = seqs[order], lens[order]
    with torch.no_grad():
        e = emb(x).transpose(0, 1)
        packed = torch.nn.utils.rnn.pack_padded_sequence(e, l)
        h0 = torch.zeros(cfg.num_layers * nd, len(l), cfg.hidden_size)
        out, _ = lstm(packed, (h0, h0.clone()))
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, padding_value=cfg.padding_value)
        assert out.shape[0] == seqs.shape[1]
        mask = x.eq(cfg.pad_idx).t().unsqueeze(-1)
        out = out.float().masked_fill(mask, float("-inf"))
        return out.max(dim=0)[0][torch.argsort(order)]


def _ragged(n, lo, hi, vocab, pad, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n,), generator=g)
    lens[int(torch.randint(0, n, (1,), generator=g))] = hi
    x = torch.randint(3, vocab, (n, hi), generator=g)
    for i, l in enumerate(lens.tolist()):
        x[i, l:] = pad
    return x, lens


@pytest.fixture(scope="module")
def full():
    from sonar_amd.laser2 import Laser2Model

    cfg = _full_cfg()
    sd = _random_state_dict(cfg)
    return cfg, sd, Laser2Model(cfg, sd, device=DEV)


def test_full_width_ragged_64(full):
    cfg, sd, model = full
    x, lens = _ragged(64, 1, 128, cfg.vocabulary_size, cfg.pad_idx, seed=1)
    got, ref = model(x, lens).cpu(), cpu_laser2(cfg, sd, x, lens)
    c, a = _assert_close(got, ref, "64 x 1..128")
    # the normalised cosine matrix, the quantity the reference's integration test asserts
    gn, rn = F.normalize(got.double()), F.normalize(ref.double())
    sim_g, sim_r = gn @ gn.T, rn @ rn.T
    worst = ((sim_g - sim_r).abs() - 1e-4 * sim_r.abs()).max().item()
    assert worst <= 1e-4, worst
    print(f"64 ragged rows: max 1-cos {c:.2e}, max |d| {a:.2e}, cosine matrix max |d| {(sim_g - sim_r).abs().max().item():.2e}")


def test_full_width_300_rows(full):
    """300 rows: crosses the 128-row recurrence tiles and many active-row boundaries."""
    cfg, sd, model = full
    x, lens = _ragged(300, 1, 96, cfg.vocabulary_size, cfg.pad_idx, seed=2)
    c, a = _assert_close(model(x, lens.to(DEV)), cpu_laser2(cfg, sd, x, lens), "300 rows")
    print(f"300 rows: max 1-cos {c:.2e}, max |d| {a:.2e}")


def test_full_width_1000_tokens(full):
    cfg, sd, model = full
    g = torch.Generator().manual_seed(3)
    x = torch.randint(3, cfg.vocabulary_size, (1, 1000), generator=g)
    lens = torch.tensor([1000])
    c, a = _assert_close(model(x.to(DEV), lens), cpu_laser2(cfg, sd, x, lens), "1000 tokens")
    print(f"1000-token sentence: 1-cos {c:.2e}, max |d| {a:.2e}")


def test_batch_independence_order_and_determinism(full):
    cfg, sd, model = full
    x, lens = _ragged(48, 1, 40, cfg.vocabulary_size, cfg.pad_idx, seed=4)
    ref = model(x, lens)
    again = model(x, lens)
    assert torch.equal(ref, again), "two identical calls differ"
    perm = torch.randperm(48, generator=torch.Generator().manual_seed(5))
    pout = model(x[perm], lens[perm])
    _assert_close(pout, ref[perm], "permuted batch")
    identical = 0
    for i in range(0, 48, 6):
        l = int(lens[i])
        alone = model(x[i:i + 1, :l], lens[i:i + 1])
        _assert_close(alone, ref[i:i + 1], f"row {i} alone")
        identical += int(torch.equal(alone, ref[i:i + 1]))
    print(f"rows alone bit-identical to their batch rows: {identical} / 8; permuted batch bit-identical: "
          f"{torch.equal(pout, ref[perm])}")


def test_chunked_forward_equals_one_call(full):
    """A batch larger than the workspace runs in row chunks, each cut to its own width; rows with non-pad tokens beyond
    their length keep the padding_value rule of the full width."""
    from sonar_amd.laser2 import Laser2Model

    cfg, sd, model = full
    x, lens = _ragged(40, 1, 50, cfg.vocabulary_size, cfg.pad_idx, seed=6)
    x[3, int(lens[3]):] = 17  # non-pad tokens beyond the length
    small = Laser2Model(cfg, sd, device=DEV, max_batch_tokens=200)
    _assert_close(small(x, lens), model(x, lens), "chunked")
    _assert_close(small(x, lens), cpu_laser2(cfg, sd, x, lens), "chunked vs cpu")


def test_out_of_vocabulary_raises_then_recovers(full):
    cfg, sd, model = full
    x, lens = _ragged(4, 2, 6, cfg.vocabulary_size, cfg.pad_idx, seed=8)
    good = model(x, lens)
    bad = x.clone()
    bad[1, 0] = cfg.vocabulary_size + 5
    with pytest.raises(IndexError):
        model(bad, lens)
    bad[1, 0] = -3
    with pytest.raises(IndexError):
        model(bad, lens)
    assert torch.equal(model(x, lens), good)


def test_argument_errors_on_device(full):
    cfg, sd, model = full
    x = torch.tensor([[5, 6, 7], [8, 9, 1]])
    with pytest.raises(ValueError):
        model(x, torch.tensor([2, 2]))
    with pytest.raises(ValueError):
        model(x, torch.tensor([3, 0]))


def test_predict_equals_tokenize_and_forward(tmp_path):
    import sentencepiece as spm

    from sonar_amd.inference_pipelines.text import collate
    from sonar_amd.laser2 import Laser2Model, Laser2TextEmbedder, Laser2Tokenizer

    corpus = tmp_path / "c.txt"
    corpus.write_text("\n".join(["to be or not to be", "i want to go biking", "je veux faire du velo"] * 40))
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "toy"), vocab_size=30, model_type="unigram",
                                   hard_vocab_limit=False, unk_id=0, bos_id=1, eos_id=2, pad_id=-1, minloglevel=2)
    tok = Laser2Tokenizer(tmp_path / "toy.model")
    fx = torch.load(GOLDEN, weights_only=True)
    case = fx["cases"][2]
    model = Laser2Model(_cfg(case), _fixture_state_dict(case), device=DEV)
    sents = ["to be or not to be", "être ou ne pas être", "i want to go biking", "je veux faire du vélo", "be"]
    emb = Laser2TextEmbedder(model, tok).predict(sents, batch_size=2)
    enc = tok.create_encoder()
    want = []
    for i in range(0, len(sents), 2):
        b = collate([enc(s) for s in sents[i:i + 2]], pad_value=1)
        want.append(model(b["seqs"], b["seq_lens"]))
    assert torch.equal(emb, torch.cat(want))
    assert emb.shape == (5, 2 * case["config"]["hidden_size"]) and emb.dtype == torch.float32


def test_reference_cosine_matrix_with_released_files():
    """tests/integration_tests/test_laser2_text.py:28-67 of the reference, with its expected values."""
    d = os.environ.get("SONAR_CHECKPOINT_DIR", "")
    if not (d and os.path.isfile(os.path.join(d, "laser2.pt")) and os.path.isfile(os.path.join(d, "laser2.spm"))):
        pytest.skip("laser2.pt and laser2.spm are not in $SONAR_CHECKPOINT_DIR")
    from sonar_amd.laser2 import Laser2TextEmbedder

    sentences = ["to be or not to be", "être ou ne pas être", "i want to go biking", "je veux faire du vélo"]
    emb = Laser2TextEmbedder("laser2_text_encoder", device=DEV).predict(sentences, batch_size=4)
    n = F.normalize(emb.float().cpu())
    expected = torch.tensor([[1.0000, 0.9614, 0.4412, 0.3923],
                             [0.9614, 1.0000, 0.4110, 0.3935],
                             [0.4412, 0.4110, 1.0000, 0.6960],
                             [0.3923, 0.3935, 0.6960, 1.0000]])
    torch.testing.assert_close(n @ n.T, expected, rtol=1e-4, atol=1e-4)
