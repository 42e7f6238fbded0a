"""CPU: the LASER2 encoder's host side -- config and card against the reference's registration, the tokenizer's id rule,
checkpoint layouts, argument validation and the refusal of a CPU device (no GPU needed)."""
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "laser2_reference.pt")


def _fixture():
    return torch.load(GOLDEN, weights_only=True)


def _small_cfg():
    from sonar_amd.laser2 import Laser2Config

    return Laser2Config(vocabulary_size=30, pad_idx=1, model_dim=8, hidden_size=6, num_layers=2, bidirectional=True)


def _small_sd(cfg):
    from sonar_amd.laser2 import _lstm_keys

    sd = {"embed_tokens.weight": torch.randn(cfg.vocabulary_size, cfg.model_dim)}
    for group in _lstm_keys(cfg):
        for k, shape in group:
            sd[k] = torch.randn(shape)
    return sd


def test_config_equals_the_reference_registration():
    """get_laser2_config("laser2") == the values the reference's own `register_laser2_configs` returns
    (models/laser2_text/config.py:23-38, executed by tests/golden/make_golden_laser2.py)."""
    import dataclasses

    from sonar_amd.laser2 import get_laser2_config

    reg = _fixture()["registration"]
    assert set(reg) == {"laser2"}
    assert dataclasses.asdict(get_laser2_config("laser2")) == reg["laser2"]
    with pytest.raises(ValueError):
        get_laser2_config("laser3")


def test_card_resolution(tmp_path, monkeypatch):
    from sonar_amd import cards

    rec = _fixture()["card"]
    assert rec["name"] == "laser2_text_encoder" and rec["model_arch"] == "laser2"
    monkeypatch.setenv("SONAR_CHECKPOINT_DIR", str(tmp_path))
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    assert cards.is_card_name(rec["name"])
    with pytest.raises(FileNotFoundError, match=rec["checkpoint"]):
        cards.resolve_card(rec["name"])
    (tmp_path / rec["checkpoint"]).write_bytes(b"x")
    (tmp_path / rec["tokenizer"]).write_bytes(b"x")
    r = cards.resolve_card(rec["name"])
    assert r.checkpoint == tmp_path / rec["checkpoint"] and r.arch == rec["model_arch"]
    assert r.tokenizer == tmp_path / rec["tokenizer"]
    assert cards.resolve_tokenizer(rec["name"]) == tmp_path / rec["tokenizer"]
    assert cards.resolve_checkpoint(rec["name"], "x") == (tmp_path / rec["checkpoint"], "laser2")


def test_tokenizer_id_rule(tmp_path):
    """fairseq2 behaviour restated, not pinned to the reference: SentencePieceEncoder(suffix_tokens=["</s>"]) appends the
    model's `</s>` id; Laser2Encoder then maps every id >= 3 to id + 4 (tokenizer.py:33-36, 80-86)."""
    import sentencepiece as spm

    from sonar_amd.laser2 import Laser2Tokenizer

    corpus = tmp_path / "c.txt"
    corpus.write_text("\n".join(["to be or not to be", "i want to go biking", "hello world"] * 40))
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "toy"), vocab_size=30, model_type="unigram",
                                   hard_vocab_limit=False, unk_id=0, bos_id=1, eos_id=2, pad_id=-1, minloglevel=2)
    tok = Laser2Tokenizer(tmp_path / "toy.model")
    sp = tok.sp
    assert tok.vocab_info.pad_idx == 1 and tok.vocab_info.size == sp.get_piece_size() + 1
    enc = tok.create_encoder()
    for s in ("to be or not to be", "hello zzz", ""):
        raw = sp.encode(s) + [sp.piece_to_id("</s>")]
        want = [i + 4 if i >= 3 else i for i in raw]
        got = enc(s)
        assert got.dtype == torch.int64 and got.tolist() == want
        assert got[-1].item() == 2   # </s> keeps its id
    assert 0 in enc("zzz").tolist()  # <unk> stays 0
    batch = tok.encode_batch(["to be", "hello world", "zzz"])
    assert [b.tolist() for b in batch] == [enc(s).tolist() for s in ("to be", "hello world", "zzz")]


def test_checkpoint_layouts():
    from sonar_amd.laser2 import laser2_state_dict

    cfg = _small_cfg()
    sd = _small_sd(cfg)
    for ckpt in (sd, {"model": sd}, {"params": {"num_embeddings": 30, "padding_idx": 1, "embed_dim": 8, "hidden_size": 6,
                                                "num_layers": 2, "bidirectional": True}, "model": sd}):
        out = laser2_state_dict(ckpt, cfg)
        assert set(out) == set(sd) and all(out[k] is sd[k] for k in sd)
    with pytest.raises(ValueError, match="hidden_size"):
        laser2_state_dict({"params": {"hidden_size": 7}, "model": sd}, cfg)
    missing = dict(sd)
    del missing["lstm.weight_hh_l1_reverse"]
    with pytest.raises(KeyError, match="lstm.weight_hh_l1_reverse"):
        laser2_state_dict(missing, cfg)
    bad = dict(sd)
    bad["lstm.weight_ih_l1"] = torch.randn(24, 6)   # layer 1 takes [h_fwd | h_bwd] = 12 inputs
    with pytest.raises(ValueError, match="lstm.weight_ih_l1"):
        laser2_state_dict(bad, cfg)
    with pytest.raises(ValueError):
        laser2_state_dict([1, 2], cfg)


def test_checkpoint_file_round_trip(tmp_path):
    from sonar_amd.laser2 import laser2_state_dict

    cfg = _small_cfg()
    sd = _small_sd(cfg)
    torch.save({"model": sd}, tmp_path / "laser2.pt")
    out = laser2_state_dict(tmp_path / "laser2.pt", cfg)
    assert all(torch.equal(out[k], sd[k]) for k in sd)


def test_argument_validation_before_device_work():
    from sonar_amd.laser2 import check_batch

    x = torch.tensor([[5, 6, 7], [8, 9, 1]])
    assert check_batch(x, torch.tensor([3, 2]), 1).tolist() == [3, 2]
    assert check_batch(x, [3, 2], 1).dtype == torch.int32
    with pytest.raises(ValueError, match="at least one token"):
        check_batch(x, torch.tensor([3, 0]), 1)
    with pytest.raises(ValueError, match="differs"):    # the reference asserts max(seq_lens) == seqs.size(1)
        check_batch(x, torch.tensor([2, 2]), 1)
    with pytest.raises(ValueError, match="entries"):
        check_batch(x, torch.tensor([3]), 1)
    with pytest.raises(ValueError, match="2-D"):
        check_batch(x[0], torch.tensor([3]), 1)
    with pytest.raises(ValueError, match="integer"):
        check_batch(x.float(), torch.tensor([3, 2]), 1)
    # the reference raises AssertionError on the width mismatch, as recorded by running it
    assert all(c["width_mismatch_asserts"] for c in _fixture()["cases"])


def test_cpu_device_refused():
    from sonar_amd.laser2 import Laser2Model

    cfg = _small_cfg()
    with pytest.raises(RuntimeError, match="HIP device only"):
        Laser2Model(cfg, _small_sd(cfg), device="cpu")
