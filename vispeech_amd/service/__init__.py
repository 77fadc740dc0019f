"""Service wrappers around the synthesis path.

The reference's web app (``inference_api.py:13, 35-65``) guards its one model with a NON-BLOCKING lock: a request
that arrives while another is being synthesised is answered "busy" at once (``mutex.acquire(blocking=False)``,
:37), otherwise ``infer`` runs and the waveform is written as a 44.1 kHz PCM16 WAV (:50).  ``SynthesisService``
(``single``) keeps those semantics -- one synthesis in flight per model, callers are refused rather than queued -- and
adds what the MI355X path makes possible: the vocoder output is STREAMED, chunk by chunk, as PCM16 bytes
(``vsp_generator_stream_chunk``: the 13/14-frame-halo streamer, bit-identical to the one-shot waveform), so the
first audio leaves after one chunk instead of after the whole utterance.  ``batching`` and ``streaming`` hold the services
that serve many callers' requests in one batch; ``_pcm`` is what all of them deliver with.  Pure host logic; all
arithmetic runs in libvispeech_hip through ``vispeech_amd.models.SynthesizerTrn``.
"""
from ._pcm import Busy, _host_i16, pcm16
from .batching import BatchingSynthesisService
from .single import PooledSynthesisService, SynthesisService
from .streaming import LiveConversion, StreamingBatchService
