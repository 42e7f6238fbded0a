"""CPU: step processor classes, their resolution for the engine, and the CPU restatement the GPU tests compare against."""
import pytest
import torch

from tests.step_processors_ref import bans, banned_seq_bans, beam_search_with_bans, ngram_bans, repeated_ngrams


def test_constructor_errors():
    from sonar_amd.generation import BannedSequenceProcessor, NGramRepeatBlockProcessor

    with pytest.raises(ValueError):
        NGramRepeatBlockProcessor(0)
    with pytest.raises(ValueError):
        NGramRepeatBlockProcessor(-2)
    with pytest.raises(ValueError):
        BannedSequenceProcessor([])
    with pytest.raises(ValueError):
        BannedSequenceProcessor([[5, 6], []])
    assert BannedSequenceProcessor([torch.tensor([5, 6]), [7]]).banned_seqs == ((5, 6), (7,))
    assert NGramRepeatBlockProcessor(3).ngram_size == 3


def test_hand_worked_ban_lists():
    # prompt [3, 7] counts: n = 2 at sequence [3, 7, 9, 7] bans what followed the earlier 7
    assert ngram_bans([3, 7, 9, 7], 2) == {9}
    # n = 1 bans every token present, the prompt's </s> (3) included
    assert ngram_bans([3, 7, 9], 1) == {3, 7, 9}
    # nothing while L < n; n = L: the only window is the sequence itself minus its last position
    assert ngram_bans([3, 7], 3) == set()
    assert ngram_bans([5, 5, 5], 3) == {5}
    assert ngram_bans([1, 2, 3, 1, 2], 3) == {3}
    # banned sequences: length 1 always, longer ones by their prefix; a prefix longer than the sequence never matches
    assert banned_seq_bans([3, 7], [[11]]) == {11}
    assert banned_seq_bans([3, 7], [[7, 12], [9, 13]]) == {12}
    assert banned_seq_bans([7], [[3, 7, 14]]) == set()
    assert banned_seq_bans([3, 7], [[3, 7, 14]]) == {14}
    assert bans([3, 7, 7], 2, [[20]]) == {7, 20}


def test_resolve_step_processors():
    from sonar_amd.generation import BannedSequenceProcessor, NGramRepeatBlockProcessor, resolve_step_processors

    assert resolve_step_processors(None) == (0, [])
    assert resolve_step_processors([NGramRepeatBlockProcessor(4), NGramRepeatBlockProcessor(2)]) == (2, [])
    assert resolve_step_processors([BannedSequenceProcessor([[1, 2]]), BannedSequenceProcessor([[9]]),
                                    NGramRepeatBlockProcessor(3)]) == (3, [[1, 2], [9]])

    class NGramRepeatBlockProcessor_:   # noqa: N801  a look-alike named like fairseq2's class
        pass

    look = type("NGramRepeatBlockProcessor", (), {"ngram_size": 5})()
    ban = type("BannedSequenceProcessor", (), {"banned_seqs": [torch.tensor([4, 8])]})()
    # fairseq2's own layout: right-aligned prefixes with a mask, last tokens apart
    fs2 = type("BannedSequenceProcessor", (), {"_banned_prefix": torch.tensor([[0, 6], [0, 0]]),
                                               "_banned_prefix_mask": torch.tensor([[0, 1], [0, 0]]),
                                               "_banned_tokens": torch.tensor([7, 9])})()
    assert resolve_step_processors([look, ban, fs2]) == (5, [[4, 8], [6, 7], [9]])
    with pytest.raises(NotImplementedError, match="NGramRepeatBlockProcessor"):
        resolve_step_processors([NGramRepeatBlockProcessor_()])


@pytest.fixture(scope="module")
def model():
    from oracle import text_decoder as OD

    ocfg = OD.OracleTextDecoderConfig(model_dim=256, num_layers=2, num_heads=4, ffn_inner_dim=512, vocab_size=1000,
                                      max_seq_len=64)
    params = OD.make_synthetic_params(ocfg, seed=4321, std=0.09)
    emb = torch.randn(3, 256, generator=torch.Generator().manual_seed(5)) * 0.3
    return OD, ocfg, params, emb


def test_helper_without_processors_is_the_oracle(model):
    OD, ocfg, params, emb = model
    kw = dict(beam_size=5, max_gen_len=(0, 20))
    m_ref, m_got = [], []
    ref = OD.beam_search_incremental(params, ocfg, emb, [3, 7], margins_out=m_ref, **kw)
    got = beam_search_with_bans(params, ocfg, emb, [3, 7], margins_out=m_got, **kw)
    assert m_ref == m_got
    for hr, hg in zip(ref, got):
        assert [h.seq.tolist() for h in hr] == [h.seq.tolist() for h in hg]
        assert [h.score for h in hr] == [h.score for h in hg]


@pytest.mark.parametrize("n", [1, 2, 3])
def test_blocking_removes_repeats_and_bites(model, n):
    OD, ocfg, params, emb = model
    kw = dict(beam_size=5, max_gen_len=(0, 30))
    plain = beam_search_with_bans(params, ocfg, emb, [3, 7], **kw)
    blocked = beam_search_with_bans(params, ocfg, emb, [3, 7], ngram=n, **kw)
    for hp, hb in zip(plain, blocked):
        for h in hb:
            full = [3, 7] + h.seq.tolist()
            # the final EOS is forced at the length cap: leave it out when n = 1 (the prompt's </s> is a repeat then)
            body = full[:-1] if full[-1] == 3 else full
            assert repeated_ngrams(body, n) == 0, (n, full)
        assert [h.seq.tolist() for h in hp] != [h.seq.tolist() for h in hb]
