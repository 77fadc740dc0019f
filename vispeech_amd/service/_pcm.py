"""What every service shares on the way out: the device-to-host copies and quantisers, the step from a float row to
PCM16, the numeric-range check after a copy, and ``Busy``."""
from __future__ import annotations

import numpy as np


def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def pcm16(audio) -> np.ndarray:
    """float waveform in [-1, 1] -> little-endian int16 (the conversion of ``utils.write_wav``)."""
    return np.clip(np.rint(np.asarray(_host(audio), dtype=np.float32).reshape(-1) * 32767.0), -32768, 32767).astype("<i2")


def _host_i16(y, flat: bool = True) -> np.ndarray:
    """int16 output of the engine's output stage -> little-endian int16 on the host (one copy): flattened, or with
    ``flat=False`` the [B, n] block as it is."""
    a = _host(y)
    return np.ascontiguousarray(a.reshape(-1) if flat else a, dtype="<i2")


def _row_pcm16(x, eng=None) -> np.ndarray:
    """One utterance's valid float samples ``x`` [1, n] -> its PCM16: the host quantiser, or with ``eng`` (a service with an
    output stage passes its engine) the engine's output stage, so that int16 at the output rate is what crosses to the host."""
    return pcm16(x) if eng is None else _host_i16(eng.output(x, pcm=True)[0])


def _check_numerics(net) -> None:
    """After a device -> host copy: raise if a kernel reported values outside the range the split-f16 matrix kernels
    represent (Engine.check_numerics; the audio just copied would be inf / NaN garbage)."""
    eng = getattr(net, "_engine", None)
    if eng is not None and hasattr(eng, "check_numerics"):
        eng.check_numerics(sync=False)


class Busy(RuntimeError):
    """Another synthesis is in flight (the reference answers such a request with a 'server busy' text)."""
