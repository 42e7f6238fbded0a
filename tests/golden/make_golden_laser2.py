"""Generate tests/golden/laser2_reference.pt by RUNNING THE REFERENCE'S OWN CODE in this container:

  * `LaserLstmEncoder` from /root/reference/sonar/nn/laser_lstm_encoder.py (plain torch, imported by path), on small
    synthetic weights, over batches that exercise its packing, padding and pooling rules;
  * the `laser2` registration of /root/reference/sonar/models/laser2_text/config.py, executed with a recording stand-in for
    fairseq2's RuntimeContext / config registry;
  * the name / arch / checkpoint / tokenizer fields of sonar/cards/laser2_text_encoder.yaml (file names of its URLs).

Weights are stored as int8 codes times one power-of-two scale per case, so they are exact in fp16 and the fixture stays
small; it holds tensors and plain containers only (loads with weights_only=True).
Run in the build container:  python tests/golden/make_golden_laser2.py
"""
import dataclasses
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True   # importing the reference by path must not leave __pycache__ in /root/reference

import torch

REF = "/root/reference/sonar"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "laser2_reference.pt")


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Registry:
    def __init__(self):
        self.archs = {}

    def decorator(self, name):
        def wrap(fn):
            self.archs[name] = fn
            return fn
        return wrap


class Context:
    def __init__(self):
        self.registries = {}

    def get_config_registry(self, kls):
        return self.registries.setdefault(kls.__name__, Registry())


def registration():
    for pkg in ("fairseq2",):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    ctx_mod = types.ModuleType("fairseq2.context")
    ctx_mod.RuntimeContext = Context
    sys.modules["fairseq2.context"] = ctx_mod
    cfg = load("ref_laser2_config", f"{REF}/models/laser2_text/config.py")
    ctx = Context()
    cfg.register_laser2_configs(ctx)
    return {name: dataclasses.asdict(fn()) for name, fn in ctx.registries["Laser2Config"].archs.items()}


def card():
    out = {}
    for line in open(f"{REF}/cards/laser2_text_encoder.yaml"):
        line = line.split("#", 1)[0].strip()
        if ":" in line:
            k, v = line.split(":", 1)
            out[k.strip()] = v.strip().strip('"')
    return {"name": out["name"], "model_arch": out["model_arch"], "checkpoint": out["checkpoint"].rsplit("/", 1)[-1],
            "tokenizer": out["tokenizer"].rsplit("/", 1)[-1]}


def batches(vocab, pad, g):
    """(name, seqs, seq_lens): the shapes the reference's packing / pooling rules act on."""
    def rnd(n, s):
        return torch.randint(3, vocab, (n, s), generator=g)

    out = []
    # ragged, Collater-style (pad after the length), unsorted, tied lengths
    lens = torch.tensor([5, 9, 3, 9, 1, 5, 7], dtype=torch.int64)
    x = rnd(len(lens), int(lens.max()))
    for i, l in enumerate(lens.tolist()):
        x[i, l:] = pad
    out.append(("ragged", x, lens))
    # all rows of equal length
    out.append(("equal", rnd(4, 6), torch.full((4,), 6, dtype=torch.int64)))
    # length-1 rows
    out.append(("len1", rnd(3, 1), torch.ones(3, dtype=torch.int64)))
    # a pad_idx token inside a row's valid length (pools -inf at that position whatever seq_lens says)
    x = rnd(3, 5)
    x[0, 2] = pad
    x[1, 0] = pad
    lens = torch.tensor([5, 4, 5], dtype=torch.int64)
    x[1, 4] = pad
    out.append(("pad_inside", x, lens))
    # non-pad tokens beyond a row's length (those positions pool padding_value)
    x = rnd(3, 4)
    lens = torch.tensor([2, 4, 3], dtype=torch.int64)
    x[2, 3] = pad
    out.append(("tail_tokens", x, lens))
    return out


def main():
    enc_mod = load("ref_laser_lstm_encoder", f"{REF}/nn/laser_lstm_encoder.py")
    g = torch.Generator().manual_seed(20261016)
    cases = []
    for name, vocab, embed, hidden, layers, bidir, pvals in (
            ("uni_1layer", 40, 32, 32, 1, False, (0.0,)),
            ("bi_2layer_odd", 37, 24, 20, 2, True, (0.0,)),
            ("bi_3layer", 50, 48, 64, 3, True, (0.0, -0.5))):
        pad = 1
        m = enc_mod.LaserLstmEncoder(num_embeddings=vocab, padding_idx=pad, embed_dim=embed, hidden_size=hidden,
                                     num_layers=layers, bidirectional=bidir).eval()
        # weights uniform in about +-1/sqrt(H) (nn.LSTM's own init range), on a 1/256 grid: int8 codes
        lim = max(1, int(round(256 / hidden ** 0.5)))
        scale = 1.0 / 256
        codes = {}
        with torch.no_grad():
            for k, p in m.state_dict().items():
                c = torch.randint(-lim, lim + 1, p.shape, generator=g, dtype=torch.int64)
                if k == "embed_tokens.weight":
                    c = torch.randint(-127, 128, p.shape, generator=g, dtype=torch.int64)
                    c[pad] = 0   # nn.Embedding(padding_idx) initialises the pad row to zero
                codes[k] = c.to(torch.int8)
                p.copy_(c.float() * scale)
        runs = []
        for pv in pvals:
            m.padding_value = pv
            for bname, x, lens in batches(vocab, pad, g):
                with torch.no_grad():
                    y = m(x, lens)
                assert torch.isfinite(y).all(), (name, bname)
                runs.append({"batch": bname, "padding_value": pv, "seqs": x.clone(), "seq_lens": lens.clone(),
                             "out": y.clone()})
        # the reference's assertion at :86
        x, lens = batches(vocab, pad, g)[0][1:]
        try:
            m(x[:, :], lens.clamp(max=int(lens.max()) - 1))
            asserts = False
        except AssertionError:
            asserts = True
        cases.append({"name": name, "config": {"vocabulary_size": vocab, "pad_idx": pad, "model_dim": embed,
                                               "hidden_size": hidden, "num_layers": layers, "bidirectional": bidir},
                      "scale": scale, "codes": codes, "runs": runs, "width_mismatch_asserts": asserts})
    out = {"registration": registration(), "card": card(), "cases": cases}
    torch.save(out, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", out["registration"], out["card"])


if __name__ == "__main__":
    main()
