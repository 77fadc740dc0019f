"""Phoneme-ID front door: the callers' side of the path.

The reference maps cleaned phoneme strings to ids with a 519-entry table (``text/symbols.py:39``:
"_" + zh + ja + en + punctuation) and stores training/inference rows as
``spk|id|phones|durations|f0|energy`` (``data_utils.py:52, 94-102``; fields space separated).  The
table is the reference's DATA and is not duplicated here: pass the list (``from text.symbols import
symbols`` in a checkout of the reference, or a JSON/text file with one symbol per line) to
``SymbolTable``.  Everything else -- id lookup, row parsing, padding a list of rows into the tensors
``SynthesizerTrn.infer`` takes -- is implemented here.
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np


class SymbolTable:
    def __init__(self, symbols: Sequence[str]):
        self.symbols = list(symbols)
        if len(set(self.symbols)) != len(self.symbols):
            raise ValueError("duplicate symbols")
        self._id: Dict[str, int] = {s: i for i, s in enumerate(self.symbols)}

    @classmethod
    def from_file(cls, path: str) -> "SymbolTable":
        text = open(path, encoding="utf-8").read()
        if path.endswith(".json"):
            return cls(json.loads(text))
        return cls([l.rstrip("\n") for l in text.splitlines() if l != ""])

    def __len__(self) -> int:
        return len(self.symbols)

    def cleaned_text_to_sequence(self, cleaned_text: Iterable[str]) -> List[int]:
        """reference text/__init__.py:9-17 (KeyError on unknown symbols, like the reference)."""
        return [self._id[s] for s in cleaned_text]


@dataclass
class FilelistRow:
    speaker: str
    utt_id: str
    phones: List[str]
    # None: the request leaves this control to the model's predictor (a plain "this text, this voice" request, what the
    # reference's inference.py:44 / inference_api.py:46 / gui.py:99 send) -- each of the three on its own
    durations: Optional[np.ndarray] = None   # int frames per phoneme (MFA, hop 512)
    f0: Optional[np.ndarray] = None          # Hz per phoneme (0 = unvoiced)
    energy: Optional[np.ndarray] = None


def request_row(speaker: str, phones: Sequence[str], durations=None, f0=None, energy=None, utt_id: str = "") -> FilelistRow:
    """A synthesis request: speaker and phones, and whichever of durations / f0 / energy the caller brings (None: predicted)."""
    arr = lambda a, dt: None if a is None else np.asarray(a, dtype=dt)
    row = FilelistRow(speaker, utt_id, list(phones), arr(durations, np.int64), arr(f0, np.float32), arr(energy, np.float32))
    for name, a in (("durations", row.durations), ("f0", row.f0), ("energy", row.energy)):
        if a is not None and len(a) != len(row.phones):
            raise ValueError(f"{name}: {len(a)} entries for {len(row.phones)} phones")
    return row


def parse_filelist_row(line: str) -> FilelistRow:
    """``spk|id|phones|durations|f0|energy`` (reference data_utils.py:52, 94-102)."""
    parts = line.rstrip("\n").split("|")
    if len(parts) != 6:
        raise ValueError(f"expected 6 '|'-separated fields, got {len(parts)}")
    spk, uid, phones, durs, f0s, ens = parts
    ph = phones.split(" ")
    d = np.array([int(x) for x in durs.split(" ")], dtype=np.int64)
    f0 = np.array([float(x) for x in f0s.strip().split(" ")], dtype=np.float32)
    en = np.array([float(x) for x in ens.strip().split(" ")], dtype=np.float32)
    if not (len(ph) == len(d) == len(f0) == len(en)):      # the reference asserts the same (data_utils.py:90-91)
        raise ValueError("phones / durations / f0 / energy lengths differ")
    return FilelistRow(spk, uid, ph, d, f0, en)


def format_filelist_row(row: FilelistRow) -> str:
    """The line ``parse_filelist_row`` reads: ``spk|id|phones|durations|f0|energy``, fields space separated, F0 and energy
    as ``'{:.3f}'`` (reference f0energy.py:99-116) -- what data preparation writes for every training recording once
    ``SynthesizerTrn.prosody_from_audio`` has produced the two tensors.  The row must carry all three controls."""
    n = len(row.phones)
    for name, a in (("durations", row.durations), ("f0", row.f0), ("energy", row.energy)):
        if a is None or len(a) != n:
            raise ValueError(f"{name}: a filelist row carries one value per phone ({n})")
    for name, s in (("speaker", row.speaker), ("utt_id", row.utt_id), *(("phone", p) for p in row.phones)):
        if "|" in s or "\n" in s or (name == "phone" and (" " in s or s == "")):
            raise ValueError(f"{name} {s!r} cannot be written into a filelist row")
    nums = lambda a: " ".join("{:.3f}".format(float(v)) for v in a)
    return "|".join([row.speaker, row.utt_id, " ".join(row.phones), " ".join(str(int(d)) for d in row.durations),
                     nums(row.f0), nums(row.energy)])


def collate_rows(rows: Sequence[FilelistRow], table: SymbolTable, spk2id: Dict[str, int]):
    """Pad rows into the arrays ``SynthesizerTrn.infer`` takes with control tensors:
    phonemes [B,Tp] int64, lengths [B], sid [B], duration / f0 / energy [B,Tp] float32 (zero padded), and
    given [B,3] bool: whether the row carries its durations / f0 / energy (a missing field is left zero; rows that carry
    all three give the arrays they always gave)."""
    B = len(rows)
    tp = max(len(r.phones) for r in rows)
    out = dict(phonemes=np.zeros((B, tp), np.int64), lengths=np.zeros(B, np.int64), sid=np.zeros(B, np.int64),
               duration=np.zeros((B, tp), np.float32), f0=np.zeros((B, tp), np.float32),
               energy=np.zeros((B, tp), np.float32), given=np.zeros((B, 3), bool))
    for b, r in enumerate(rows):
        n = len(r.phones)
        out["phonemes"][b, :n] = table.cleaned_text_to_sequence(r.phones)
        out["lengths"][b] = n
        out["sid"][b] = spk2id[r.speaker]
        for k, (key, a) in enumerate((("duration", r.durations), ("f0", r.f0), ("energy", r.energy))):
            if a is not None:
                out[key][b, :n] = a
                out["given"][b, k] = True
    return out
