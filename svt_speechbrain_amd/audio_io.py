"""Wav files in and out, with the sample conversion on the GPU: what ``torchaudio.info`` / ``load`` / ``save`` and
``speechbrain.dataio.dataio.read_audio`` / ``write_audio`` (``speechbrain/dataio/dataio.py:161-211, 291-320``) do for the RIFF/WAVE files
every entry point of the reference starts from (``MIR_ST500/prepare_benchmarks.py:58``, ``N20EMv2/audio_visual/synthesis_noise.py``,
``MIR_ST500/train_audio_ssl.py:376``).

* ``info``: the header alone (``svt_wav_parse``, host code: PCM at 8 / 16 / 24 / 32 bits, IEEE float at 32 / 64, plain or
  WAVE_FORMAT_EXTENSIBLE, 1..8 channels; compressed and big-endian containers are refused).
* ``load``: reads the header prefix, then ONLY the bytes of the requested frames, into a pinned staging buffer; one asynchronous copy of
  the raw PCM and one ``svt_pcm_decode`` launch (``csrc/pcm.hip``) on the current stream give the planar fp32 tensor.  A 16-bit file
  crosses PCIe at 2 bytes per sample instead of 4, and a 5 s utterance of a 4-minute song costs 5 s of file, not 4 minutes.
* ``save``: one ``svt_pcm_encode`` launch, one copy to the host, header and data written in one go.

Value rule of ``load`` (torchaudio's ``normalize=True`` conventions, as far as they can be known without torchaudio; ``normalize=False``
is not offered): the fp32 nearest, ties to even, to ``(b - 128) / 128`` (8-bit), ``x / 2**15``, ``x / 2**23``, ``x / 2**31`` (so
``INT32_MAX`` gives 1.0), the bits of a float32 unchanged, a float64 rounded once.  No bit parity with sox is claimed for 32-bit integer
and 64-bit float files.  ``save`` writes float32 bits unchanged (what ``torchaudio.save`` does with a float32 tensor) or, with
``encoding="PCM_S", bits_per_sample=16``, ``clamp(rint(x * 32768), -32768, 32767)`` with ties to even and NaN -> 0 (soundfile's
``PCM_16``); no parity with sox's rounding is claimed.

The tensors live on the GPU; there is no CPU fallback.  The staging buffer is per device and is not thread-safe.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import Dict, Optional, Tuple

import torch

from . import _lib

# include/svt_mi355.h: svt_pcm_format, SVT_WAV_NEED_MORE, SVT_PCM_FRAMES_PER_WORKGROUP / SVT_PCM_MAX_WORKGROUPS (a call with more frames
# than their product sends its workgroups on a second trip)
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = 1, 2, 3, 4, 5, 6
NEED_MORE = 1
FRAMES_PER_WORKGROUP = 4096
MAX_WORKGROUPS = 1024
HEADER_PREFIX = 4096   # bytes of the first read; svt_wav_parse asks for more when a long LIST / bext chunk precedes the data

_ENCODING = {PCM_U8: "PCM_U", PCM_S16: "PCM_S", PCM_S24: "PCM_S", PCM_S32: "PCM_S", PCM_F32: "PCM_F", PCM_F64: "PCM_F"}

AudioMetaData = namedtuple("AudioMetaData", ["sample_rate", "num_frames", "num_channels", "bits_per_sample", "encoding"])

_open = open   # the one way this module opens a file (binary): tests count the bytes read through it


def _parse(fh, path) -> _lib.WavInfoC:
    """The header of an open file: a prefix of HEADER_PREFIX bytes, longer as long as the parser asks for more."""
    lib = _lib.load()
    size = os.fstat(fh.fileno()).st_size if hasattr(fh, "fileno") else os.path.getsize(path)
    head = fh.read(min(HEADER_PREFIX, size))
    wi, need = _lib.WavInfoC(), C.c_int64(0)
    while True:
        rc = lib.svt_wav_parse(head, len(head), size, C.byref(wi), C.byref(need))
        if rc != NEED_MORE:
            break
        more = fh.read(need.value - len(head))
        if not more:
            raise _lib.SvtError(f"{path}: the file ended while its header was read")
        head += more
    _lib.check(rc, str(path), lib)
    return wi


def info(path) -> AudioMetaData:
    """``torchaudio.info``: ``sample_rate, num_frames, num_channels, bits_per_sample, encoding`` ("PCM_U" 8-bit, "PCM_S", "PCM_F")."""
    with _open(path, "rb") as fh:
        wi = _parse(fh, path)
    return AudioMetaData(wi.sample_rate, wi.frames, wi.channels, wi.bits_per_sample, _ENCODING[wi.format])


class _Staging:
    """The pinned buffer the file's bytes pass through, reused from call to call.  The copy that reads it is asynchronous, so an event
    recorded behind that copy is waited for before the next file overwrites the buffer."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.sent: Optional[torch.cuda.Event] = None

    def take(self, nbytes: int) -> torch.Tensor:
        if self.sent is not None:
            self.sent.synchronize()
            self.sent = None
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(1 << 20, -(-nbytes // (1 << 20)) << 20), dtype=torch.uint8, pin_memory=True)
        return self.buf

    def mark_sent(self, device) -> None:
        self.sent = torch.cuda.Event()
        self.sent.record(torch.cuda.current_stream(device))


_staging: Dict[torch.device, _Staging] = {}


def _device(device) -> torch.device:
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise _lib.SvtError("wav files are decoded on the GPU; there is no CPU fallback")
    return torch.device("cuda", _lib.dev_index(device))


@torch.no_grad()
def load(path, frame_offset: int = 0, num_frames: int = -1, channels_first: bool = True, device=None) -> Tuple[torch.Tensor, int]:
    """``torchaudio.load`` of a wav file: ``(fp32 tensor (channels, frames) on the GPU, sample_rate)``; ``(frames, channels)`` with
    ``channels_first=False``.  ``num_frames < 0``: to the end.  An offset at or past the end gives an empty tensor and no launch."""
    device = _device(device)
    frame_offset = int(frame_offset)
    if frame_offset < 0:
        raise ValueError("frame_offset must not be negative")
    with _open(path, "rb") as fh:
        wi = _parse(fh, path)
        n = max(0, wi.frames - frame_offset)
        if num_frames >= 0:
            n = min(n, int(num_frames))
        out = torch.empty((wi.channels, n), dtype=torch.float32, device=device)
        if n:
            nbytes = n * wi.block_align
            stage = _staging.setdefault(device, _Staging())
            pinned = stage.take(nbytes)
            fh.seek(wi.data_offset + frame_offset * wi.block_align)
            got = fh.readinto(memoryview(pinned.numpy())[:nbytes])
            if got != nbytes:
                raise _lib.SvtError(f"{path}: {got} of {nbytes} bytes read")
            raw = torch.empty(nbytes, dtype=torch.uint8, device=device)
            with torch.cuda.device(device):
                raw.copy_(pinned[:nbytes], non_blocking=True)
                stage.mark_sent(device)
                lib = _lib.load()
                _lib.check(lib.svt_pcm_decode(_lib.ptr(raw), wi.format, wi.channels, n, _lib.ptr(out), n, 0, device.index,
                                              _lib.stream_ptr(device)), "svt_pcm_decode", lib)
    return (out if channels_first else out.t()), wi.sample_rate


def _format_of(encoding, bits_per_sample) -> int:
    if encoding in (None, "PCM_F") and bits_per_sample in (None, 32):
        return PCM_F32
    if encoding == "PCM_S" and bits_per_sample in (None, 16):
        return PCM_S16
    raise ValueError(f"save writes 32-bit float (the default) or encoding='PCM_S', bits_per_sample=16; got {encoding!r}, {bits_per_sample!r}")


@torch.no_grad()
def save(path, src: torch.Tensor, sample_rate: int, channels_first: bool = True, encoding: Optional[str] = None,
         bits_per_sample: Optional[int] = None) -> None:
    """``torchaudio.save`` of a wav file: ``src`` is a 2-D fp32 tensor on the GPU, ``(channels, frames)`` (or ``(frames, channels)`` with
    ``channels_first=False``).  The default writes the float32 file; ``encoding="PCM_S", bits_per_sample=16`` the 16-bit one."""
    fmt = _format_of(encoding, bits_per_sample)
    if src.dim() != 2:
        raise ValueError(f"expected a 2-D tensor, got {tuple(src.shape)}")
    if src.dtype != torch.float32:
        raise ValueError(f"expected a float32 tensor, got {src.dtype}")
    if not src.is_cuda:
        raise _lib.SvtError("wav files are encoded on the GPU; there is no CPU fallback")
    x = src.detach() if channels_first else src.detach().t()
    channels, n = x.shape
    if n and (x.stride(1) != 1 or (channels > 1 and x.stride(0) < n)):
        x = x.contiguous()
    lib = _lib.load()
    head = (C.c_ubyte * 64)()
    head_bytes = C.c_int64(0)
    _lib.check(lib.svt_wav_header(fmt, channels, int(sample_rate), n, head, 64, C.byref(head_bytes)), "svt_wav_header", lib)
    data = b""
    if n:
        raw = torch.empty(n * channels * (4 if fmt == PCM_F32 else 2), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.svt_pcm_encode(_lib.ptr(x), x.stride(0) if channels > 1 else n, channels, n, fmt, _lib.ptr(raw),
                                          _lib.dev_index(x.device), _lib.stream_ptr(x.device)), "svt_pcm_encode", lib)
            data = memoryview(raw.cpu().numpy())
    with _open(path, "wb") as fh:
        fh.write(bytes(head[:head_bytes.value]))
        fh.write(data)


def read_audio(waveforms_obj, device=None) -> torch.Tensor:
    """``speechbrain.dataio.dataio.read_audio``: a path, or ``{"file": path, "start": first frame, "stop": one past the last}`` (a
    missing ``stop`` reads to the end).  ``(samples,)`` for a mono file, ``(samples, channels)`` otherwise, on the GPU."""
    if isinstance(waveforms_obj, (str, os.PathLike)):
        audio, _ = load(waveforms_obj, device=device)
    else:
        start = int(waveforms_obj.get("start", 0))
        stop = waveforms_obj.get("stop")
        audio, _ = load(waveforms_obj["file"], frame_offset=start, num_frames=-1 if stop is None else max(0, int(stop) - start),
                        device=device)
    return audio.transpose(0, 1).squeeze(1)


def write_audio(filepath, audio: torch.Tensor, samplerate: int) -> None:
    """``speechbrain.dataio.dataio.write_audio``: ``audio`` is ``(samples,)`` or ``(samples, channels)`` on the GPU; a float32 file."""
    if audio.dim() == 2:
        audio = audio.transpose(0, 1)
    elif audio.dim() == 1:
        audio = audio.unsqueeze(0)
    save(filepath, audio, samplerate)
