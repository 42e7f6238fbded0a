"""LASER2 BiLSTM text encoder on the MI355X engine, with the reference's interfaces.

  * `Laser2Config`, `get_laser2_config("laser2")`: sonar/models/laser2_text/config.py:12-38.
  * `Laser2Tokenizer(path)`: sonar/models/laser2_text/tokenizer.py:27-97 -- SentencePiece ids, `</s>` appended, then
    `id + 4` for every id >= 3 (the fairseq dictionary offset of the LASER vocabulary); `vocab_info.pad_idx == 1`.
  * `Laser2Model(config, state_dict, device)` -> `forward(seqs, seq_lens)`: LaserLstmEncoder.forward
    (sonar/nn/laser_lstm_encoder.py:60-116), `[n, hidden_size * (1 + bidirectional)]` fp32 on the device.
  * `load_laser2_model(card_or_path, device)`, card `laser2_text_encoder` (sonar/cards/laser2_text_encoder.yaml).
  * `Laser2TextEmbedder.predict(sentences)`: strings -> tokenizer -> Collater(pad_value=1) -> forward, the path of the
    reference's integration test (tests/integration_tests/test_laser2_text.py:28-67).

The embedding gather, the recurrence and the pooling run in `libsonar_mi355.so` (`smi_laser2_*`, sonar_amd/csrc/laser2.hip);
there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Mapping, Optional, Sequence, Union

import torch

from . import _lib
from .text_encoder import VocabularyInfo

LASER2_PAD_IDX = 1


@dataclass
class Laser2Config:
    """sonar/models/laser2_text/config.py:12-20."""

    vocabulary_size: int
    pad_idx: int
    model_dim: int = 320
    hidden_size: int = 512
    num_layers: int = 1
    bidirectional: bool = False
    padding_value: float = 0.0

    @property
    def output_units(self) -> int:
        return self.hidden_size * (2 if self.bidirectional else 1)


def get_laser2_config(arch: str) -> Laser2Config:
    """The architectures the reference registers (config.py:23-38)."""
    if arch == "laser2":
        return Laser2Config(vocabulary_size=50004, pad_idx=1, model_dim=320, hidden_size=512, num_layers=5,
                            bidirectional=True, padding_value=0.0)
    raise ValueError(f"unknown LASER2 architecture {arch!r} (laser2)")


# ---- tokenizer -------------------------------------------------------------------------------------------------------

class Laser2Tokenizer:
    """SentencePiece model + the LASER2 id rule (tokenizer.py:27-97).  fairseq2's SentencePieceModel adds `<pad>` as a
    control symbol (which only grows the vocabulary by one); the padding index of the LASER dictionary, the value the
    reference's integration test collates with, is 1."""

    def __init__(self, path: Union[str, Path]):
        import sentencepiece as spm

        self.sp = spm.SentencePieceProcessor(model_file=str(path))
        self.eos_piece_id = self.sp.piece_to_id("</s>")
        self.vocab_info = VocabularyInfo(size=self.sp.get_piece_size() + 1, unk_idx=self.sp.unk_id(),
                                         bos_idx=self.sp.bos_id(), eos_idx=self.sp.eos_id(), pad_idx=LASER2_PAD_IDX)

    @staticmethod
    def _shift(ids: List[int]) -> torch.Tensor:
        t = torch.tensor(ids, dtype=torch.int64)
        return torch.where(t >= 3, t + 4, t)

    def create_encoder(self):
        """-> callable str -> int64 tensor: pieces, `</s>`, then `where(id >= 3, id + 4, id)` (tokenizer.py:33-36, 80-86)."""
        def encode(sentence: str) -> torch.Tensor:
            return self._shift(self.sp.encode(sentence) + [self.eos_piece_id])
        return encode

    def encode_batch(self, sentences: Sequence[str], num_threads: int = 8) -> List[torch.Tensor]:
        """The encoder over many sentences with SentencePiece's multi-threaded encode (same ids)."""
        pieces = self.sp.encode(list(sentences), num_threads=num_threads)
        return [self._shift(p + [self.eos_piece_id]) for p in pieces]


# ---- checkpoint ------------------------------------------------------------------------------------------------------

# LaserLstmEncoder's constructor arguments as a fairseq / LASER checkpoint's "params" dict names them -> Laser2Config fields
_PARAMS_TO_CONFIG = {"num_embeddings": "vocabulary_size", "padding_idx": "pad_idx", "embed_dim": "model_dim",
                     "hidden_size": "hidden_size", "num_layers": "num_layers", "bidirectional": "bidirectional",
                     "padding_value": "padding_value"}


def _lstm_keys(cfg: Laser2Config):
    """(key, shape) of every nn.LSTM parameter, layer-major, forward then reverse."""
    H = cfg.hidden_size
    nd = 2 if cfg.bidirectional else 1
    for k in range(cfg.num_layers):
        in_dim = cfg.model_dim if k == 0 else nd * H
        for d in range(nd):
            sfx = f"_l{k}" + ("_reverse" if d else "")
            yield (f"lstm.weight_ih{sfx}", (4 * H, in_dim)), (f"lstm.weight_hh{sfx}", (4 * H, H)), \
                  (f"lstm.bias_ih{sfx}", (4 * H,)), (f"lstm.bias_hh{sfx}", (4 * H,))


def laser2_state_dict(checkpoint: Union[str, Path, Mapping], cfg: Laser2Config) -> Dict[str, torch.Tensor]:
    """A LASER2 checkpoint -> the state dict of LaserLstmEncoder (`embed_tokens.weight`, `lstm.{weight,bias}_{ih,hh}_l{k}
    [_reverse]`), checked against `cfg`.

    Accepts a bare state dict, `{"model": state_dict, ...}`, or a file holding either (loaded with `weights_only=True`).
    When a `"params"` dict is present (LASER's own checkpoints store the encoder's constructor arguments there), every
    field it names must equal the config.  The released `laser2.pt` cannot be inspected offline, so its exact layout is
    assumed from the reference's loader; a missing key raises KeyError naming it, a misshapen one ValueError."""
    if isinstance(checkpoint, (str, Path)):
        checkpoint = torch.load(str(checkpoint), map_location="cpu", weights_only=True)
    if not isinstance(checkpoint, Mapping):
        raise ValueError(f"a LASER2 checkpoint is a state dict or {{'model': state dict}}, not {type(checkpoint).__name__}")
    params = checkpoint.get("params")
    if isinstance(params, Mapping):
        for pk, field in _PARAMS_TO_CONFIG.items():
            if pk in params:
                want = getattr(cfg, field)
                got = type(want)(params[pk]) if not isinstance(want, bool) else bool(params[pk])
                if got != want:
                    raise ValueError(f"checkpoint params[{pk!r}] = {params[pk]!r} does not match the config's {field} = {want!r}")
    sd = checkpoint["model"] if "model" in checkpoint and isinstance(checkpoint["model"], Mapping) else checkpoint
    out: Dict[str, torch.Tensor] = {}
    expect = [("embed_tokens.weight", (cfg.vocabulary_size, cfg.model_dim))]
    for group in _lstm_keys(cfg):
        expect.extend(group)
    for key, shape in expect:
        if key not in sd:
            raise KeyError(f"LASER2 checkpoint: missing key {key!r}")
        t = sd[key]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"LASER2 checkpoint: {key!r} has shape {got}, expected {shape}")
        out[key] = t
    return out


# ---- model -----------------------------------------------------------------------------------------------------------

def check_batch(seqs: torch.Tensor, seq_lens, pad_idx: int) -> torch.Tensor:
    """Argument checks of forward(), before any device work -> host int32 lengths.  The reference asserts
    max(seq_lens) == seqs.size(1) (laser_lstm_encoder.py:86); here that, and a zero length, are ValueErrors."""
    if not isinstance(seqs, torch.Tensor) or seqs.dim() != 2:
        raise ValueError("seqs must be a 2-D [batch, seq_len] tensor of token ids")
    if seqs.dtype.is_floating_point or seqs.dtype == torch.bool:
        raise ValueError(f"seqs must hold integer token ids, not {seqs.dtype}")
    n, s = seqs.shape
    if n == 0 or s == 0:
        raise ValueError(f"empty batch {tuple(seqs.shape)}")
    lens = torch.as_tensor(seq_lens).reshape(-1)
    if lens.numel() != n:
        raise ValueError(f"seq_lens has {lens.numel()} entries for a batch of {n} rows")
    lens = lens.to("cpu", torch.int64)
    if int(lens.min()) <= 0:
        raise ValueError("every sequence needs at least one token (seq_lens > 0)")
    if int(lens.max()) != s:
        raise ValueError(f"max(seq_lens) = {int(lens.max())} differs from seqs.size(1) = {s} (the reference asserts equality)")
    return lens.to(torch.int32).contiguous()


def _tv(t: torch.Tensor, keep: list) -> _lib.smi_tensor:
    t = t.detach()
    if t.dtype not in (torch.float16, torch.float32):
        t = t.float()
    t = t.contiguous()
    keep.append(t)
    return _lib.smi_tensor(t.data_ptr(), _lib.SMI_F32 if t.dtype == torch.float32 else _lib.SMI_F16, int(t.is_cuda), t.numel())


class Laser2Model:
    """LaserLstmEncoder on the engine: `model(seqs, seq_lens)` -> fp32 `[n, output_units]` on the device.

    `seqs` (CPU or device, integer ids) and `seq_lens` (CPU or device) as the reference takes them.  Batches with more than
    `max_batch_tokens` tokens (the sum of the lengths) run in chunks of rows."""

    def __init__(self, config: Laser2Config, state_dict: Mapping[str, torch.Tensor], device="cuda",
                 max_batch_tokens: int = 1 << 18):
        self.config = config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the LASER2 MI355X engine runs on a HIP device only (no CPU path)")
        sd = laser2_state_dict(state_dict, config)
        self.lib = _lib.load()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.max_batch_tokens = int(max_batch_tokens)
        keep: list = []
        groups = list(_lstm_keys(config))
        arr = (_lib.smi_laser2_layer * len(groups))()
        for i, ((wi, _), (wh, _), (bi, _), (bh, _)) in enumerate(groups):
            arr[i].weight_ih, arr[i].weight_hh = _tv(sd[wi], keep), _tv(sd[wh], keep)
            arr[i].bias_ih, arr[i].bias_hh = _tv(sd[bi], keep), _tv(sd[bh], keep)
        emb = _tv(sd["embed_tokens.weight"], keep)
        cfg = _lib.smi_laser2_config(config.vocabulary_size, config.pad_idx, config.model_dim, config.hidden_size,
                                     config.num_layers, 1 if config.bidirectional else 0, float(config.padding_value))
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.smi_init(idx))
            _lib.check(self.lib.smi_laser2_create(C.byref(cfg), C.byref(emb), arr, 0, C.byref(self._handle)))

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            self.lib.smi_laser2_destroy(h)
            self._handle = None

    @property
    def output_units(self) -> int:
        return self.config.output_units

    def device_bytes(self) -> int:
        return int(self.lib.smi_laser2_device_bytes(self._handle))

    def check(self) -> None:
        """Synchronise the current stream; IndexError if a batch held out-of-vocabulary ids (nn.Embedding raises there)."""
        with torch.cuda.device(self.device):
            rc = self.lib.smi_laser2_status(self._handle, _lib.current_stream_ptr())
        if rc != _lib.SMI_OK:
            raise IndexError(self.lib.smi_last_error().decode("utf-8", "replace"))

    def _run(self, ids: torch.Tensor, lens: torch.Tensor, out: torch.Tensor) -> None:
        n, s = ids.shape
        lp = lens.data_ptr()
        _lib.check(self.lib.smi_laser2_forward(self._handle, ids.data_ptr(), C.cast(lp, C.POINTER(C.c_int32)), n, s,
                                               out.data_ptr(), _lib.current_stream_ptr()))

    def forward(self, seqs: torch.Tensor, seq_lens) -> torch.Tensor:
        lens = check_batch(seqs, seq_lens, self.config.pad_idx)
        n, s = seqs.shape
        with torch.cuda.device(self.device):
            ids = seqs.to(self.device, torch.int64).contiguous()
            out = torch.empty(n, self.output_units, dtype=torch.float32, device=self.device)
            if int(lens.sum()) <= self.max_batch_tokens:
                self._run(ids, lens, out)
            else:
                self._forward_chunked(ids, lens, out)
            self.check()
        return out

    __call__ = forward

    def _forward_chunked(self, ids: torch.Tensor, lens: torch.Tensor, out: torch.Tensor) -> None:
        """Rows in chunks of at most max_batch_tokens tokens.  Each chunk is cut to its own longest row; a row that has
        non-pad tokens between that width and the batch's still pools padding_value with them (the reference pads every
        row to the batch width)."""
        n, s = ids.shape
        order = torch.argsort(lens.to(torch.int64), descending=True, stable=True)
        start = 0
        while start < n:
            stop, tok = start, 0
            while stop < n and (stop == start or tok + int(lens[order[stop]]) <= self.max_batch_tokens):
                tok += int(lens[order[stop]])
                stop += 1
            rows = order[start:stop]
            cl = lens[rows].contiguous()
            w = int(cl.max())
            rows_d = rows.to(ids.device)
            sub = ids.index_select(0, rows_d)
            part = torch.empty(len(rows), self.output_units, dtype=torch.float32, device=ids.device)
            self._run(sub[:, :w].contiguous(), cl, part)
            if w < s:
                cut = (sub[:, w:] != self.config.pad_idx).any(dim=1, keepdim=True)
                part = torch.where(cut, part.clamp_min(self.config.padding_value), part)
            out.index_copy_(0, rows_d, part)
            start = stop


def load_laser2_model(card_or_path: Union[str, Path, Mapping] = "laser2_text_encoder", device="cuda",
                      arch: str = "laser2", max_batch_tokens: int = 1 << 18) -> Laser2Model:
    """The model hub's `load("laser2_text_encoder")`: a card name (file under $SONAR_CHECKPOINT_DIR), a path, or an
    in-memory checkpoint."""
    from .cards import resolve_checkpoint

    cfg = get_laser2_config(arch)
    if isinstance(card_or_path, Mapping):
        return Laser2Model(cfg, card_or_path, device, max_batch_tokens)
    path, arch = resolve_checkpoint(card_or_path, arch)
    return Laser2Model(get_laser2_config(arch), laser2_state_dict(path, cfg), device, max_batch_tokens)


class Laser2TextEmbedder:
    """strings -> Laser2Tokenizer -> Collater(pad_value=1) -> Laser2Model, one call (test_laser2_text.py:28-67)."""

    def __init__(self, encoder: Union[str, Path, Laser2Model] = "laser2_text_encoder",
                 tokenizer: Union[str, Path, Laser2Tokenizer, None] = None, device="cuda"):
        from .cards import resolve_tokenizer

        self.model = encoder if isinstance(encoder, Laser2Model) else load_laser2_model(encoder, device)
        if tokenizer is None:
            tokenizer = "laser2_text_encoder"
        self.tokenizer = tokenizer if isinstance(tokenizer, Laser2Tokenizer) else Laser2Tokenizer(resolve_tokenizer(tokenizer))

    def predict(self, sentences: Sequence[str], batch_size: int = 32) -> torch.Tensor:
        from .inference_pipelines.text import collate

        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        sentences = list(sentences)
        if not sentences:
            return torch.empty(0, self.model.output_units, dtype=torch.float32, device=self.model.device)
        toks = self.tokenizer.encode_batch(sentences)
        outs = []
        for i in range(0, len(toks), batch_size):
            b = collate(toks[i:i + batch_size], pad_value=LASER2_PAD_IDX)
            outs.append(self.model(b["seqs"], b["seq_lens"]))
        return torch.cat(outs, dim=0)
