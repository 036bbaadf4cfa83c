"""A small Motion-JPEG AVI writer with an optional 16-bit PCM sound track (reference: moviepy's ImageSequenceClip(...).write_videofile, which
needs ffmpeg).  Frames are encoded with PIL's JPEG encoder and written as they arrive, the sound interleaved frame by frame; ``close`` appends
the ``idx1`` index and patches the RIFF sizes and frame counts written as placeholders at the start.

    RIFF 'AVI '  LIST 'hdrl' ( avih, LIST 'strl' ( strh vids/MJPG, strf BITMAPINFOHEADER ) [, LIST 'strl' ( strh auds, strf WAVEFORMAT ) ] )
                 LIST 'movi' ( 00dc ... [01wb ...] )  idx1
"""
from __future__ import annotations

import io
import struct
from typing import Optional

import numpy as np

AVIF_HASINDEX, AVIF_ISINTERLEAVED, AVIIF_KEYFRAME = 0x10, 0x100, 0x10


def pcm16(waveform) -> np.ndarray:
    """Float samples in [-1, 1] (or int16 samples) -> int16, (n,) or (n, channels)."""
    a = np.asarray(waveform)
    if a.dtype == np.int16:
        return a
    return np.round(np.clip(a.astype(np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)


def jpeg_size(jpeg: bytes):
    """(width, height) of a baseline JPEG file, from its SOF0 segment; ValueError when the bytes do not start with SOI or carry no SOF0 before
    the scan."""
    if len(jpeg) < 4 or jpeg[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file: no SOI marker at the start")
    pos = 2
    while pos + 4 <= len(jpeg) and jpeg[pos] == 0xFF:
        marker, size = jpeg[pos + 1], struct.unpack(">H", jpeg[pos + 2:pos + 4])[0]
        if marker == 0xC0 and pos + 9 <= len(jpeg):
            height, width = struct.unpack(">HH", jpeg[pos + 5:pos + 9])
            return width, height
        if marker == 0xDA:
            break
        pos += 2 + size
    raise ValueError("not a baseline JPEG file: no SOF0 segment before the scan")


class AviWriter:
    """``write(frame)`` takes (height, width, 3) uint8 images, B-G-R unless ``bgr=False``.  ``audio``: int16 samples, (n,) or (n, channels), at
    ``audio_rate`` Hz; whatever lies past the last frame is written at ``close``."""

    def __init__(self, path: str, fps: float, width: int, height: int, audio: Optional[np.ndarray] = None, audio_rate: Optional[int] = None,
                 quality: int = 90, bgr: bool = True):
        if fps <= 0 or width < 1 or height < 1:
            raise ValueError("fps, width and height must be positive")
        self.fps, self.width, self.height, self.quality, self.bgr = float(fps), int(width), int(height), int(quality), bgr
        self.audio = None
        if audio is not None:
            if not audio_rate or audio_rate <= 0:
                raise ValueError("audio needs its sampling rate")
            a = pcm16(audio)
            self.audio = np.ascontiguousarray(a.reshape(len(a), -1)).astype("<i2")
            self.audio_rate, self.channels = int(audio_rate), self.audio.shape[1]
        self.frames = 0
        self.audio_pos = 0          # samples written so far
        self.index = []             # (fourcc, offset from the 'movi' fourcc, size)
        self.max_chunk = [0, 0]
        self.f = open(path, "wb")
        self._write_header()

    # ---- layout
    def _strh(self, fcc_type: bytes, handler: bytes, scale: int, rate: int, length: int, suggested: int, sample_size: int, frame) -> bytes:
        return struct.pack("<4s4sIHHIIIIIIiI4h", fcc_type, handler, 0, 0, 0, 0, scale, rate, 0, length, suggested, -1, sample_size, *frame)

    def _chunk(self, fourcc: bytes, data: bytes) -> bytes:
        return fourcc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")

    def _list(self, kind: bytes, data: bytes) -> bytes:
        return b"LIST" + struct.pack("<I", len(data) + 4) + kind + data

    def _header(self, riff_size: int, movi_size: int) -> bytes:
        scale, rate = 1000, int(round(self.fps * 1000))
        streams = 2 if self.audio is not None else 1
        byte_rate = (self.audio_rate * self.channels * 2) if self.audio is not None else 0
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), byte_rate + self.max_chunk[0] * int(np.ceil(self.fps)), 0, AVIF_HASINDEX | AVIF_ISINTERLEAVED,
                           self.frames, 0, streams, self.max_chunk[0], self.width, self.height, 0, 0, 0, 0)
        bih = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        hdrl = self._chunk(b"avih", avih) + self._list(b"strl", self._chunk(b"strh", self._strh(b"vids", b"MJPG", scale, rate, self.frames, self.max_chunk[0],
                                                                                             0, (0, 0, self.width, self.height))) + self._chunk(b"strf", bih))
        if self.audio is not None:
            align = self.channels * 2
            wfx = struct.pack("<HHIIHH", 1, self.channels, self.audio_rate, byte_rate, align, 16)
            hdrl += self._list(b"strl", self._chunk(b"strh", self._strh(b"auds", b"\0\0\0\0", align, byte_rate, self.audio_pos, self.max_chunk[1], align,
                                                                       (0, 0, 0, 0))) + self._chunk(b"strf", wfx))
        return b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + self._list(b"hdrl", hdrl) + b"LIST" + struct.pack("<I", movi_size + 4) + b"movi"

    def _write_header(self) -> None:
        h = self._header(0, 0)
        self.f.write(h)
        self.movi_start = len(h) - 4   # offset of the 'movi' fourcc: idx1 offsets count from it

    def _put(self, stream: int, fourcc: bytes, data: bytes) -> None:
        self.index.append((fourcc, self.f.tell() - self.movi_start, len(data)))
        self.max_chunk[stream] = max(self.max_chunk[stream], len(data))
        self.f.write(self._chunk(fourcc, data))

    # ---- streams
    def _audio_until(self, end: int) -> None:
        end = min(end, len(self.audio))
        if end > self.audio_pos:
            self._put(1, b"01wb", self.audio[self.audio_pos:end].tobytes())
            self.audio_pos = end

    def write(self, frame: np.ndarray) -> None:
        from PIL import Image
        a = np.asarray(frame)
        if a.shape != (self.height, self.width, 3) or a.dtype != np.uint8:
            raise ValueError(f"frame must be ({self.height}, {self.width}, 3) uint8, got {a.shape} {a.dtype}")
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a[..., ::-1] if self.bgr else a), "RGB").save(buf, format="JPEG", quality=self.quality)
        self._put(0, b"00dc", buf.getvalue())
        self.frames += 1
        if self.audio is not None:
            self._audio_until(int(round(self.frames * self.audio_rate / self.fps)))

    def write_encoded(self, jpeg: bytes) -> None:
        """A frame that is already a JPEG file (said_amd.render.JpegEncoder): what ``write`` does after its encode step.  The file must start
        with SOI and its SOF0 must carry the writer's width and height."""
        size = jpeg_size(jpeg)
        if size != (self.width, self.height):
            raise ValueError(f"the JPEG is {size[0]} x {size[1]}, the video {self.width} x {self.height}")
        self._put(0, b"00dc", bytes(jpeg))
        self.frames += 1
        if self.audio is not None:
            self._audio_until(int(round(self.frames * self.audio_rate / self.fps)))

    def close(self) -> None:
        if self.f is None:
            return
        if self.audio is not None:
            self._audio_until(len(self.audio))
        movi_size = self.f.tell() - self.movi_start - 4
        self.f.write(self._chunk(b"idx1", b"".join(struct.pack("<4sIII", fcc, AVIIF_KEYFRAME, off, size) for fcc, off, size in self.index)))
        end = self.f.tell()
        self.f.seek(0)
        self.f.write(self._header(end - 8, movi_size))   # same length as the placeholder: only counts and sizes change
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
