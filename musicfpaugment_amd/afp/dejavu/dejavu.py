"""Dejavu on MI355X -- drop-in for afp/dejavu/dejavu.py (Dejavu, read, unique_hash).

Fingerprints come from the device chain of fingerprint.py, the database is the device store and matcher of database.py
(DESIGN.md §3.9).  The reference loads its Demucs checkpoint at import time (:34-43) and its UNet inside fingerprint.py;
here the networks are handed to the constructor (`unet=` for denoising_model "unet", `demucs=` for "demucs").  Two
instances share one database when it is passed as `config["database"]`, as two reference instances share one Postgres
server; any other value there (the reference's connection options) gives the instance a database of its own.
"""
from __future__ import annotations

from hashlib import sha1
from itertools import groupby
from time import time
from typing import Dict, List, Tuple

import torch

from ...constants import afp_settings
from .database import DeviceDatabase
from .fingerprint import fingerprint

TOPN = 1               # afp/dejavu/variables.py
MIN_HASHES = 1
SONG_ID, SONG_NAME, OFFSET, OFFSET_SECS = "song_id", "song_name", "offset", "offset_seconds"
INPUT_HASHES, FINGERPRINTED_HASHES, HASHES_MATCHED = "input_total_hashes", "fingerprinted_hashes_in_db", "hashes_matched_in_input"
INPUT_CONFIDENCE, INPUT_CONFIDENCE_2, FINGERPRINTED_CONFIDENCE = "input_confidence", "input_confidence_2", "fingerprinted_confidence"


def unique_hash(file_path: str, block_size: int = 2 ** 20) -> str:
    """Upper-case hex SHA-1 of the file's bytes (dejavu.py:46-66)."""
    s = sha1()
    with open(file_path, "rb") as f:
        for buf in iter(lambda: f.read(block_size), b""):
            s.update(buf)
    return s.hexdigest().upper()


def read(filename: str, denoising: bool = False, denoising_model: str = "unet", *, demucs=None, device="cuda"):
    """dejavu.py:69-118 for .pkl at 8 kHz and .wav at any rate (resampled to 8 kHz on the device like the reference's torchaudio
    Resample, :91-115): ([samples x 32767], samplerate, unique_hash).  With denoising_model
    "demucs" the waveform goes through `demucs` first (:95-103); the UNet acts later, inside fingerprint()."""
    from ..audfprint.peak_extractor import Audfprint_peaks
    if denoising is True:
        assert denoising_model in ["demucs", "unet"]
    sr = afp_settings["dejavu"]["samplerate"]
    audio = Audfprint_peaks._read_waveform(filename, sr).to(device)
    if denoising is True and denoising_model == "demucs":
        if demucs is None:
            raise ValueError("denoising_model='demucs' needs the demucs module")
        with torch.no_grad():
            audio = demucs(audio.reshape(1, -1))[0, 0]
    return [audio * 32767], sr, unique_hash(filename)


class Dejavu:
    def __init__(self, config, settings, state="set", denoising=False, denoising_model=None, *, unet=None, demucs=None,
                 device="cuda"):
        self.config = config
        self.settings = settings
        self.device = torch.device(device)
        db = (config or {}).get("database")
        self.db = db if isinstance(db, DeviceDatabase) else DeviceDatabase(device=self.device)
        self.denoising = denoising
        self.denoising_model = denoising_model
        if self.denoising is True:
            assert self.denoising_model in ["unet", "demucs"]
            if (unet if denoising_model == "unet" else demucs) is None:
                raise ValueError(f"denoising_model={denoising_model!r} needs the {denoising_model} module")
        self.unet, self.demucs = unet, demucs
        if state == "set":
            self.db.setup()
        elif state == "clear":
            self.db.empty()
        self._load_fingerprinted_audio_hashes()

    def _load_fingerprinted_audio_hashes(self) -> None:
        self.songs = self.db.get_songs()
        self.songhashes_set = {song["file_sha1"] for song in self.songs}

    def fingerprint_directory(self, mp3_path_list: list, nprocesses: int = None) -> None:
        """dejavu.py:154-225: fingerprint every file not yet known by its SHA-1, one song per file, in list order."""
        for filename in mp3_path_list:
            if unique_hash(filename) in self.songhashes_set:
                continue
            song_name, hashes, file_hash = self._fingerprint_worker((filename, None))
            sid = self.db.insert_song(song_name, file_hash, len(hashes))
            self.db.insert_hashes(sid, hashes)
            self.db.set_song_fingerprinted(sid)
            self._load_fingerprinted_audio_hashes()

    @staticmethod
    def _fingerprint_worker(arguments):
        import os
        file_name = arguments[0]
        song_name, _ = os.path.splitext(os.path.basename(file_name))
        fingerprints, file_hash = Dejavu.get_file_fingerprints(file_name, print_output=False)
        return song_name, fingerprints, file_hash

    @staticmethod
    def get_file_fingerprints(file_name: str, print_output: bool = False):
        """dejavu.py:239-253: the SET of (hash, offset) pairs of every channel, without denoising."""
        channels, fs, file_hash = read(file_name)
        fingerprints = set()
        for channel in channels:
            fingerprints |= set(fingerprint(channel, Fs=fs, device=channel.device))
        return fingerprints, file_hash

    def generate_fingerprints(self, samples, get_masks: bool = False):
        """dejavu.py:255-289: (hashes, seconds) of one channel, or (peak_mask, specgram) of a FILE with get_masks=True."""
        Fs = self.settings["samplerate"]
        t = time()
        kw = dict(Fs=Fs, denoising=self.denoising, denoising_model=self.denoising_model, unet=self.unet, device=self.device)
        if get_masks is True:
            channels, _, _ = read(samples, denoising=self.denoising, denoising_model=self.denoising_model, demucs=self.demucs,
                                  device=self.device)
            _, peak_mask, specgram = fingerprint(channels[0], get_masks=True, **kw)
            return peak_mask, specgram
        hashes = fingerprint(samples, get_masks=get_masks, **kw)
        return hashes, time() - t

    def find_matches(self, hashes) -> Tuple[List[Tuple[int, int]], Dict[int, int], float]:
        t = time()
        matches, dedup_hashes = self.db.return_matches(hashes)
        return matches, dedup_hashes, time() - t

    def align_matches(self, matches, dedup_hashes: Dict[int, int], queried_hashes: int, topn: int = TOPN) -> List[Dict]:
        """dejavu.py:312-378: the count of every (sid, diff); per song its first maximum in (sid, diff) order; songs by that
        count, descending and stable; the first `topn`.  Every row reports the FIRST song's count as nb_matches_with_offset
        and input_confidence_2, as the reference does."""
        counted = [(key[0], key[1], sum(1 for _ in grp)) for key, grp in groupby(sorted(matches), key=lambda m: (m[0], m[1]))]
        best = []
        for _, grp in groupby(counted, key=lambda c: c[0]):
            top = None
            for c in grp:
                if top is None or c[2] > top[2]:
                    top = c
            best.append(top)
        best.sort(key=lambda c: c[2], reverse=True)
        out = []
        for song_id, offset, _ in best[:topn]:
            song = self.db.get_song_by_id(song_id)
            song_hashes = song.get("total_hashes", None)
            hashes_matched = dedup_hashes[song_id]
            out.append({
                SONG_ID: song_id,
                SONG_NAME: song.get(SONG_NAME, None).encode("utf8"),
                INPUT_HASHES: queried_hashes,
                FINGERPRINTED_HASHES: song_hashes,
                HASHES_MATCHED: hashes_matched,
                INPUT_CONFIDENCE: round(hashes_matched / queried_hashes, 2),
                INPUT_CONFIDENCE_2: round(best[0][2] / queried_hashes, 2),
                "nb_matches_with_offset": best[0][2],
                FINGERPRINTED_CONFIDENCE: round(hashes_matched / song_hashes, 2),
                OFFSET: offset,
                OFFSET_SECS: round(float(offset) / self.settings["samplerate"] * self.settings["n_hop"], 5),
                "file_sha1": (song.get("file_sha1", None) or "").encode("utf8"),
            })
        return out
