"""Dejavu's file recognizer on MI355X -- drop-in for afp/dejavu/file_recognizer.py (BaseRecognizer, FileRecognizer)."""
from __future__ import annotations

from time import time
from typing import Dict

import numpy as np

from ...constants import afp_settings
from .dejavu import MIN_HASHES, read


class BaseRecognizer(object):
    def __init__(self, dejavu):
        self.dejavu = dejavu
        self.Fs = afp_settings["dejavu"]["samplerate"]

    def _recognize(self, *data):
        """file_recognizer.py:17-34: the SET of the channels' (hash, offset) pairs, matched and aligned."""
        fingerprint_times = []
        hashes = set()
        for channel in data:
            fingerprints, fingerprint_time = self.dejavu.generate_fingerprints(channel)
            fingerprint_times.append(fingerprint_time)
            hashes |= set(fingerprints)
        matches, dedup_hashes, query_time = self.dejavu.find_matches(hashes)
        t = time()
        final_results = self.dejavu.align_matches(matches, dedup_hashes, len(hashes))
        return final_results, np.sum(fingerprint_times), query_time, time() - t

    def recognize(self, *args) -> Dict:
        raise NotImplementedError


class FileRecognizer(BaseRecognizer):
    def recognize_file(self, filename: str) -> Dict:
        """file_recognizer.py:42-72: a match needs nb_matches_with_offset > MIN_HASHES."""
        channels, self.Fs, _ = read(filename, denoising=self.dejavu.denoising, denoising_model=self.dejavu.denoising_model,
                                    demucs=self.dejavu.demucs, device=self.dejavu.device)
        t = time()
        matches, fingerprint_time, query_time, align_time = self._recognize(*channels)
        t = time() - t
        is_match = bool(len(matches)) and matches[0]["nb_matches_with_offset"] > MIN_HASHES
        return {"total_time": t, "fingerprint_time": fingerprint_time, "query_time": query_time, "align_time": align_time,
                "results": matches, "match": is_match}

    def recognize(self, filename: str) -> Dict:
        return self.recognize_file(filename)
