#!/usr/bin/env python3
"""Generate tests/golden/vad_chunk.npz by running the REFERENCE's own VAD_segments.VAD_chunk.

Like make_golden.py this runs only where the read-only reference is mounted at /root/reference;
the reference is imported, never copied.  webrtcvad and librosa are not needed: `webrtcvad.Vad` is
stubbed with a scripted list of per-frame decisions and `librosa.load` with the synthetic waveform,
a real 16-bit mono wav is written with the stdlib (VAD_chunk reads its bytes for the framing), and
everything after the per-frame decision -- frame_generator, vad_collector, the 0.4 s chunking and
the slicing of the audio -- is the reference's code.

Recorded per flag script <name>:
  <name>_flags   uint8 [n_frames]  the scripted decisions (one per frame frame_generator yields)
  <name>_n       int64             samples of the waveform
  <name>_times   float64 [k, 2]    VAD_chunk's speech_times
  <name>_lens    int64 [k]         len() of each of VAD_chunk's speech_segs
and `names`, the list of scripts.  tests/test_dvector_export.py compares dvector.vad_frame_count /
vad_times / voiced_ranges against them.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SR = 16000
FRAME = 320  # samples of a 20 ms frame


def scripts():
    """name -> (n_samples, flags or None): flags are cut or padded with silence to the number of
    frames the reference's frame_generator yields for n_samples."""
    rng = np.random.default_rng(20)
    base = np.zeros(400, dtype=np.uint8)
    base[30:130] = 1
    base[180:260] = 1
    base[300:400] = 1  # speech at the end of the file
    noisy = base ^ (rng.random(400) < 0.05).astype(np.uint8)
    z, v = lambda k: [0] * k, lambda k: [1] * k
    return {
        "none": (3 * SR, z(150)),
        "to_end": (4 * SR, z(25) + v(400)),                                # leftover branch
        "short10": (2 * SR, z(20) + v(10) + z(80)),                        # a span of exactly 0.4 s
        "short11": (2 * SR, z(20) + v(11) + z(80)),                        # 0.42 s: a 0.02 s last chunk
        "touching": (4 * SR + 7, z(15) + v(30) + z(10) + v(30) + z(120)),  # second span starts where the first ends
        "between": (int(3.5 * SR), z(50) + v(75) + z(60)),
        "flips": (7 * SR + 123, list(noisy)),
    }


def main():
    if not os.path.isdir(REF):
        print("reference not present; nothing to do")
        return
    import yaml
    orig = yaml.load_all
    yaml.load_all = lambda s, Loader=yaml.SafeLoader: orig(s, Loader=Loader)
    state = {}

    class Vad:
        def __init__(self, mode):
            self.it = iter(state["flags"])

        def is_speech(self, buf, sample_rate):
            assert sample_rate == SR and len(buf) == 2 * FRAME
            return bool(next(self.it))

    vad_mod, rosa = types.ModuleType("webrtcvad"), types.ModuleType("librosa")
    vad_mod.Vad = Vad
    rosa.load = lambda path, sr: (state["audio"], sr)
    sys.modules["webrtcvad"], sys.modules["librosa"] = vad_mod, rosa
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(HERE, ".."))
    import logmel_ref
    cwd = os.getcwd()
    os.chdir(REF)
    sys.path.insert(0, REF)
    try:
        import VAD_segments
    finally:
        os.chdir(cwd)
    assert VAD_segments.hp.data.sr == SR

    out = {"names": np.asarray(list(scripts()))}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (n, flags) in scripts().items():
            audio = logmel_ref.tones(n, seed=n)
            path = os.path.join(tmp, name + ".wav")
            with wave.open(path, "wb") as wf:
                wf.setnchannels(1)
                wf.setsampwidth(2)
                wf.setframerate(SR)
                wf.writeframes((audio * 32767.0).astype("<i2").tobytes())
            n_frames = len(list(VAD_segments.frame_generator(20, b"\0" * (2 * n), SR)))
            flags = (list(flags) + [0] * n_frames)[:n_frames]
            state["flags"], state["audio"] = flags, audio
            times, segs = VAD_segments.VAD_chunk(2, path)
            out[name + "_flags"] = np.asarray(flags, dtype=np.uint8)
            out[name + "_n"] = np.int64(n)
            out[name + "_times"] = np.asarray(times, dtype=np.float64).reshape(-1, 2)
            out[name + "_lens"] = np.asarray([len(s) for s in segs], dtype=np.int64)
            print(name, n, n_frames, [(float(a), float(b)) for a, b in times], [len(s) for s in segs])
    np.savez_compressed(os.path.join(HERE, "vad_chunk.npz"), **out)


if __name__ == "__main__":
    main()
