"""Teacher-forced scoring without a GPU: the C ABI entry is declared and bound, and the pipelines score the target
sequence prompt + pieces + [eos]."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_score_symbol_declared_and_bound():
    from sonar_amd import _lib

    hdr = (ROOT / "include" / "sonar_mi355.h").read_text()
    assert re.search(r"int\s+smi_text_decoder_score\s*\(", hdr)
    restype, args = _lib.SYMBOLS["smi_text_decoder_score"]
    assert restype is C.c_int and len(args) == 9
    assert args[6] is C.POINTER(C.c_int32)       # lens: host int32 [n]
    assert _lib.ABI_VERSION == 7                  # no struct changed
    lib = _lib.load()                             # every declared symbol resolves (build() ran first)
    assert lib.smi_text_decoder_score.argtypes == args


def _toy_tokenizer(tmp_path):
    spm = pytest.importorskip("sentencepiece")
    import torch

    from sonar_amd.tokenizer import NllbTokenizer

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
    return NllbTokenizer(str(tmp_path / "toy.model"))


def test_target_sequences_are_prompt_pieces_eos(tmp_path):
    from sonar_amd.inference_pipelines.text import score_sequences

    tok = _toy_tokenizer(tmp_path)
    eos = tok.vocab_info.eos_idx
    lang = tok.lang_idx("fra_Latn")
    texts = ["hello world", "", "my name is paul"]
    seqs, plen = score_sequences(tok, texts, "fra_Latn")
    assert plen == 2
    for text, s in zip(texts, seqs):
        assert s == [eos, lang] + [p + 1 for p in tok.sp.encode(text)] + [eos]
    assert seqs[1] == [eos, lang, eos]
    # the tokenizer's own target mode is unchanged: prefix [eos, lang], no suffix
    enc = tok.create_encoder(lang="fra_Latn", mode="target")
    assert enc.prefix == [eos, lang] and enc.suffix == []
    assert enc.ids("hello world") == seqs[0][:-1]
