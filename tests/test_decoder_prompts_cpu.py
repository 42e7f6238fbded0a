"""CPU: per-sentence prompts (smi_text_decoder_generate_prompts / _sample_prompts) -- the ABI, the engine's argument handling
against a stub library that records the call, and the pipeline's prompt assembly against a stub engine."""
import contextlib
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ ABI
def test_prompt_entries_declared_bound_and_exported():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sonar_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    vp, i32 = C.c_void_p, C.c_int32
    for name, params in (("smi_text_decoder_generate_prompts", _lib.smi_beam_search_params),
                         ("smi_text_decoder_sample_prompts", _lib.smi_sampling_params)):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert re.search(rf"\bT {name}\b", out), name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int
        # dec, emb, emb_dtype, n, prompts, prompt_stride, prompt_lens, gen_cap, min_gen_len, params, tokens, lens, scores, stream
        assert argtypes == [vp, vp, i32, i32, C.POINTER(C.c_int64), i32, C.POINTER(i32), i32, i32, C.POINTER(params),
                            vp, vp, vp, vp]
        decl = re.search(rf"int {name}\s*\((.*?)\);", hdr, flags=re.S).group(1)
        assert len(decl.split(",")) == len(argtypes)
        for word in ("const int64_t* prompts", "int32_t prompt_stride", "const int32_t* prompt_lens", "int32_t gen_cap",
                     "int32_t min_gen_len"):
            assert word in decl, (name, word)
    assert _lib.ABI_VERSION == 7


def test_prompt_entries_refuse_null_arguments():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    assert lib.smi_text_decoder_generate_prompts(None, None, 0, 1, None, 1, None, 1, 1, None, None, None, None, None) != 0
    assert lib.smi_text_decoder_sample_prompts(None, None, 0, 1, None, 1, None, 1, 1, None, None, None, None, None) != 0


# ------------------------------------------------------------------------------------------ engine arguments
def test_nested_and_flat_prompts_are_told_apart():
    from sonar_amd.text_decoder import split_prompts

    assert split_prompts([3, 700]) == (False, [3, 700])
    assert split_prompts((3, 700, 5)) == (False, [3, 700, 5])
    assert split_prompts(torch.tensor([3, 700])) == (False, [3, 700])
    assert split_prompts([torch.tensor(3), 700]) == (False, [3, 700])
    assert split_prompts([[3, 700], (3, 701, 9)]) == (True, [[3, 700], [3, 701, 9]])
    assert split_prompts([torch.tensor([3, 700]), [3, 701]]) == (True, [[3, 700], [3, 701]])
    assert split_prompts([[3, 700]]) == (True, [[3, 700]])
    assert split_prompts([]) == (False, [])
    with pytest.raises(ValueError, match="mixture"):
        split_prompts([3, [3, 700]])


def test_length_limits_per_row_and_errors():
    from sonar_amd.text_decoder import length_limits, plan_prompt_rows

    pr = plan_prompt_rows(64, 256, [[3, 700], [3, 701, 5, 6, 7], [3, 702, 9]], 3, 2, (0, 4), None, None)
    assert pr.lens == [2, 5, 3] and pr.stride == 5 and pr.gen_cap == 4 and pr.model_max == 64
    assert pr.limits == [(6, 4), (9, 7), (7, 5)] and pr.width == 9
    assert pr.limits == [length_limits(64, 256, L, 2, (0, 4), None, None)[:2] for L in pr.lens]
    assert pr.flat() == [3, 700, 0, 0, 0, 3, 701, 5, 6, 7, 3, 702, 9, 0, 0]
    # the model-side cap clamps each row by itself: max_len = min(plen + gen_cap, model_max), min_len <= max_len
    pr = plan_prompt_rows(64, 256, [[3, 700], [3] * 9], 2, 3, (0, 4), 10, None)
    assert pr.limits == [(6, 5), (10, 10)] and pr.width == 10 and pr.model_max == 10
    # the fairseq2 rule a * source_len + b
    assert plan_prompt_rows(64, 256, [[3, 700]], 1, 1, (1, 8), None, 5).gen_cap == 13
    assert plan_prompt_rows(64, 16, [[3, 700]], 1, 1, (1, 8), None, None).gen_cap == 24
    with pytest.raises(ValueError, match="2 prompts for 3 embeddings"):
        plan_prompt_rows(64, 256, [[3, 700], [3, 701]], 3, 1, (0, 4), None, None)
    with pytest.raises(ValueError, match="row 1"):
        plan_prompt_rows(64, 256, [[3, 700], [3] * 64, [3, 702]], 3, 1, (0, 4), None, None)
    with pytest.raises(ValueError, match="row 2"):
        plan_prompt_rows(64, 256, [[3, 700], [3, 701], [3] * 8], 3, 1, (0, 4), 8, None)
    with pytest.raises(ValueError, match="row 0 is empty"):
        plan_prompt_rows(64, 256, [[], [3, 701]], 2, 1, (0, 4), None, None)
    with pytest.raises(ValueError, match="cannot be larger"):
        plan_prompt_rows(64, 256, [[3, 700]], 1, 1, (0, 4), 65, None)
    with pytest.raises(ValueError, match="min_gen_len"):
        plan_prompt_rows(64, 256, [[3, 700]], 1, 5, (0, 4), None, None)


class _StubLib:
    """Stands in for the loaded library: records the call and returns `status`."""

    def __init__(self, status=0):
        self.calls, self.status = [], status

    def _record(self, name, args):
        dec, emb, dtype, n, prompts, stride, plens, gen_cap, min_gen, params = args[:10]
        self.calls.append(dict(name=name, n=n, stride=stride, prompts=list(prompts), lens=list(plens), gen_cap=gen_cap,
                               min_gen=min_gen, max_seq_len=params._obj.max_seq_len, dtype=dtype))
        return self.status

    def smi_text_decoder_generate_prompts(self, *a):
        return self._record("generate_prompts", a)

    def smi_text_decoder_sample_prompts(self, *a):
        return self._record("sample_prompts", a)

    def smi_text_decoder_generate(self, *a):
        self.calls.append(dict(name="generate", n=a[3], prompt=list(a[4]), plen=a[5], max_seq_len=a[6]._obj.max_seq_len,
                               min_seq_len=a[6]._obj.min_seq_len))
        return self.status

    def smi_last_error(self):
        return b"row 1: prompt token 5000 out of range"


@pytest.fixture()
def stub_engine(monkeypatch):
    from sonar_amd import _lib
    from sonar_amd.text_decoder import SonarTextDecoderConfig, TextDecoderEngine
    from sonar_amd.text_encoder import VocabularyInfo

    eng = TextDecoderEngine.__new__(TextDecoderEngine)
    eng.cfg = SonarTextDecoderConfig(model_dim=16, num_decoder_layers=1, num_decoder_attn_heads=2, ffn_inner_dim=32,
                                     vocab_info=VocabularyInfo(size=1000), max_seq_len=64)
    eng.device = torch.device("cpu")
    eng.lib = _StubLib()
    eng._handle = None
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: None)
    monkeypatch.setattr(_lib, "load", lambda: eng.lib)
    return eng


def test_engine_hands_per_sentence_prompts_to_the_new_entries(stub_engine):
    from sonar_amd import _lib
    from sonar_amd.generation import TopKSampler

    eng = stub_engine
    emb = torch.zeros(3, 16)
    prompts = [[3, 700], [3, 701, 5, 6, 7], (3, 702, 9)]
    toks, lens, scores = eng.generate(emb, prompts, beam_size=2, min_gen_len=2, max_gen_len=(0, 4))
    call = eng.lib.calls[-1]
    assert call == dict(name="generate_prompts", n=3, stride=5, prompts=[3, 700, 0, 0, 0, 3, 701, 5, 6, 7, 3, 702, 9, 0, 0],
                        lens=[2, 5, 3], gen_cap=4, min_gen=2, max_seq_len=64, dtype=_lib.SMI_F32)
    assert toks.shape == (3, 2, 9) and lens.shape == (3, 2) and scores.shape == (3, 2)
    toks, lens, scores = eng.sample(emb.half(), prompts, TopKSampler(3), max_gen_len=(0, 4), max_seq_len=8, seed=1)
    call = eng.lib.calls[-1]
    assert call["name"] == "sample_prompts" and call["max_seq_len"] == 8 and call["gen_cap"] == 4 and call["min_gen"] == 1
    assert call["dtype"] == _lib.SMI_F16 and toks.shape == (3, 8) and lens.shape == (3,)
    # a flat prompt stays on today's entry, with today's arguments
    toks, _, _ = eng.generate(emb, [3, 700], beam_size=2, min_gen_len=2, max_gen_len=(0, 4))
    assert eng.lib.calls[-1] == dict(name="generate", n=3, prompt=[3, 700], plen=2, max_seq_len=6, min_seq_len=4)
    assert toks.shape == (3, 2, 6)
    ncalls = len(eng.lib.calls)
    with pytest.raises(ValueError, match="2 prompts for 3 embeddings"):
        eng.generate(emb, prompts[:2], beam_size=2)
    with pytest.raises(ValueError, match="row 1"):
        eng.generate(emb, [[3, 700], [3] * 64, [3, 701]], beam_size=2)
    with pytest.raises(ValueError, match="row 1"):
        eng.sample(emb, [[3, 700], [3] * 64, [3, 701]], TopKSampler(3))
    assert len(eng.lib.calls) == ncalls        # refused on the host
    # what the library refuses as an invalid argument (a token outside the vocabulary) is a ValueError too
    eng.lib.status = _lib.SMI_ERR_INVALID_ARG
    with pytest.raises(ValueError, match="row 1"):
        eng.generate(emb, [[3, 700], [3, 5000], [3, 701]], beam_size=2)


# ------------------------------------------------------------------------------------------ pipeline
class _Enc:
    def __init__(self, lang_id):
        self.prefix, self.suffix = [3, lang_id], []

    def ids(self, text):
        return self.prefix + [10 + len(w) for w in text.split()]


class _Tok:
    """Target-mode tokenizer stand-in: a word is the piece 10 + its length."""
    langs = {"fra_Latn": 700, "eng_Latn": 701, "deu_Latn": 702}

    class vocab_info:
        eos_idx = 3

    def create_encoder(self, task=None, lang=None, mode=None):
        assert mode == "target"
        if lang not in self.langs:
            raise ValueError(f"`lang` must be a supported language, but is {lang!r} instead")
        return _Enc(self.langs[lang])

    def create_decoder(self):
        return lambda ids: " ".join(str(int(t)) for t in ids if int(t) >= 4)


class _Engine:
    def __init__(self):
        self.calls = []

    def generate(self, emb, prompt, **kw):
        self.calls.append(("generate", emb.shape[0], prompt, kw))
        n = emb.shape[0]
        toks = torch.full((n, 1, 4), -1, dtype=torch.int32)
        for i in range(n):   # "generate" [100 + the row's first embedding value, EOS]
            toks[i, 0, 0], toks[i, 0, 1] = 100 + int(emb[i, 0]), 3
        return toks, torch.full((n, 1), 2, dtype=torch.int32), torch.zeros(n, 1)

    def sample(self, emb, prompt, sampler, sentence_offset=0, **kw):
        self.calls.append(("sample", emb.shape[0], prompt, dict(kw, sentence_offset=sentence_offset)))
        t, l, s = self.generate(emb, prompt)
        self.calls.pop()
        return t[:, 0], l[:, 0], s[:, 0]

    def score(self, emb, seqs):
        self.calls.append(("score", emb.shape[0], [list(s) for s in seqs], {}))
        t = max(len(s) for s in seqs)
        return torch.full((emb.shape[0], t - 1), -1.0)


class _Model:
    device = torch.device("cpu")

    def __init__(self):
        self.engine = _Engine()

    def eval(self):
        return self


@pytest.fixture()
def pipe():
    from sonar_amd.inference_pipelines import EmbeddingToTextModelPipeline

    return EmbeddingToTextModelPipeline(_Model(), _Tok())


def test_pipeline_assembles_one_prompt_per_row(pipe):
    from sonar_amd.inference_pipelines.text import target_prompts

    emb = torch.arange(5, dtype=torch.float32).unsqueeze(1).repeat(1, 4)
    langs = ["fra_Latn", "eng_Latn", "fra_Latn", "deu_Latn", "eng_Latn"]
    out = pipe.predict(emb, target_lang=langs, batch_size=2, max_gen_len=(0, 9))
    calls = pipe.model.engine.calls
    assert [(c[0], c[1]) for c in calls] == [("generate", 2), ("generate", 2), ("generate", 1)]   # batches in input order
    assert [c[2] for c in calls] == [[[3, 700], [3, 701]], [[3, 700], [3, 702]], [[3, 701]]]
    assert all(c[3] == dict(max_gen_len=(0, 9)) for c in calls)
    assert out == ["100", "101", "102", "103", "104"]
    # prefixes: the pieces join the row's prompt (no EOS) and the returned text includes them
    calls.clear()
    out = pipe.predict(emb, target_lang=langs, batch_size=3, prefixes=["ab cde", None, "f", "", "gh ij klm"])
    assert [c[2] for c in calls] == [[[3, 700, 12, 13], [3, 701], [3, 700, 11]], [[3, 702], [3, 701, 12, 12, 13]]]
    assert out == ["12 13 100", "101", "11 102", "103", "12 12 13 104"]
    # one language with prefixes: the prompts still differ from row to row
    calls.clear()
    pipe.predict(emb[:2], target_lang="deu_Latn", prefixes=["ab", None])
    assert calls[0][2] == [[3, 702, 12], [3, 702]]
    # a plain string and no prefixes: the engine call of before, one flat prompt
    calls.clear()
    pipe.predict(emb[:2], target_lang="deu_Latn", batch_size=2)
    assert calls[0][2] == [3, 702]
    # the sampler path takes the same two arguments
    calls.clear()
    out = pipe.predict(emb, target_lang=langs, batch_size=2, sampler=object(), prefixes=[None, "ab", None, None, None])
    assert [c[0] for c in calls] == ["sample"] * 3 and [c[3]["sentence_offset"] for c in calls] == [0, 2, 4]
    assert calls[0][2] == [[3, 700], [3, 701, 12]] and out[1] == "12 101"
    assert target_prompts(_Tok(), 2, "eng_Latn", None) == ([[3, 701], [3, 701]], [[], []])
    for bad in (dict(target_lang=langs[:4]), dict(target_lang=langs, prefixes=["a"]), dict(target_lang="fra_Latn", prefixes=[])):
        with pytest.raises(ValueError, match="for 5 inputs"):
            pipe.predict(emb, **bad)
    with pytest.raises(ValueError, match="supported language"):
        pipe.predict(emb, target_lang=["fra_Latn"] * 4 + ["xxx_Latn"])


def test_pipeline_scores_with_one_language_per_input(pipe):
    from sonar_amd.inference_pipelines.text import score_sequences

    seqs, plen = score_sequences(_Tok(), ["ab cde", "f"], ["deu_Latn", "fra_Latn"])
    assert seqs == [[3, 702, 12, 13, 3], [3, 700, 11, 3]] and plen == 2
    assert score_sequences(_Tok(), ["ab cde", "f"], "fra_Latn") == ([[3, 700, 12, 13, 3], [3, 700, 11, 3]], 2)
    with pytest.raises(ValueError, match="1 target languages for 2 texts"):
        score_sequences(_Tok(), ["ab", "f"], ["deu_Latn"])
    emb = torch.zeros(3, 4)
    got = pipe.score(emb, ["ab cde", "f", "gh"], target_lang=["deu_Latn", "fra_Latn", "eng_Latn"], batch_size=2)
    assert got.tolist() == [-3.0, -2.0, -2.0]          # pieces + the final EOS, one stub log-probability of -1 each
    scored = sorted(s for c in pipe.model.engine.calls for s in c[2])
    assert scored == sorted([[3, 702, 12, 13, 3], [3, 700, 11, 3], [3, 701, 12, 3]])
