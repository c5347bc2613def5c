"""Hand-built DEFLATE streams for the device PNG decoder (test helper, no GPU and no project
imports): a small writer that emits exactly what it is told -- stored, fixed and dynamic blocks
whose code-length symbols, Huffman sets, matches and zlib / PNG wrapping the caller chooses -- and
the table of cases built with it, shared by ``test_deflate_cases.py`` (the table against zlib and
PIL, on the CPU) and ``test_png_device_streams.py`` (the device against the table).

zlib's encoder is one point in what RFC 1951 allows; the table holds the shapes it never emits
(repeat codes across the HLIT boundary, one-code and empty distance sets, 15-bit codes by
construction, copies and literal runs placed on the ends of the decoder's 36,864-byte ring, flush
markers, small windows) and, for every ``SLG_PNG_E_*`` status, streams that must end at one named
check of ``png_inflate_kernel`` / ``png_unfilter_kernel``.  It is the statement of what the device
decoder accepts and refuses."""
from __future__ import annotations

import functools
import random
import struct
import zlib
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

import png_encode

# include/slgpu.h (test_png_device_streams.py checks them against the package's)
OK, E_STREAM, E_SIZE, E_ADLER, E_FILTER, E_UNSUPPORTED = 0, 1, 2, 3, 4, 5
# png_device.hip: the LDS output ring, its flush block, the primary table's index bits, the widest row
RING, FLUSH, FAST_BITS, MAX_ROW = 36864, 2048, 10, 24576

EOB = 256
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 §3.2.5, as printed there
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class BitWriter:
    """LSB-first bit packing (RFC 1951 §3.1.1); Huffman codes go in most significant bit first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self) -> int:
        return 8 * len(self.out) + self.n

    def bits(self, v: int, n: int) -> None:
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, length: int) -> None:
        code &= (1 << length) - 1                      # (an over-subscribed set's codes overflow)
        self.bits(int(format(code, f"0{length}b")[::-1], 2), length)

    def align(self) -> None:
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self) -> bytes:
        self.align()
        return bytes(self.out)


def canonical(lengths) -> list:
    """RFC 1951 §3.2.2: per symbol (code, length), or None for length 0."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
        else:
            out.append((nxt[l], l))
            nxt[l] += 1
    return out


def kraft(lengths) -> Fraction:
    return sum((Fraction(1, 1 << l) for l in lengths if l), Fraction(0))


def balanced(k: int, depth: int = 0) -> list:
    """k code lengths that fill a subtree hanging ``depth`` bits down (Kraft sum 2^-depth)."""
    m = max(0, (k - 1).bit_length())
    short = (1 << m) - k
    return [depth + m - 1] * short + [depth + m] * (k - short)


def table(n: int, assign: dict) -> list:
    out = [0] * n
    for s, l in assign.items():
        out[s] = l
    return out


def expand(cl_symbols) -> list:
    """The code lengths a sequence of code-length symbols (sym, extra) stands for."""
    out = []
    for s, e in cl_symbols:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + e)
        elif s == 17:
            out += [0] * (3 + e)
        else:
            out += [0] * (11 + e)
    return out


def cl_plain(lengths) -> list:
    return [(l, 0) for l in lengths]


def cl_rle(lengths) -> list:
    """Run-length form over the whole HLIT + HDIST sequence (runs cross the boundary freely)."""
    out, i = [], 0
    while i < len(lengths):
        v, j = lengths[i], i
        while j < len(lengths) and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 3:
                r = min(run, 138)
                if r >= 11:
                    out.append((18, r - 11))
                else:
                    out.append((17, r - 3))
                run -= r
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
        out += [(v, 0)] * run
        i = j
    return out


def cl_complete(cl_symbols) -> list:
    """A complete code-length code (<= 7 bits) over the symbols used; a second symbol is given a
    code when only one is used (zlib and the RFC want this set complete)."""
    used = sorted({s for s, _ in cl_symbols})
    if len(used) == 1:
        used.append(next(s for s in range(19) if s not in used))
    return table(19, dict(zip(used, balanced(len(used)))))


def _len_code(length: int) -> int:
    return max(s for s in range(29) if LEN_BASE[s] <= length)


def _dist_code(dist: int) -> int:
    return max(d for d in range(30) if DIST_BASE[d] <= dist)


class Deflate:
    """A deflate stream under construction and the bytes it is meant to inflate to.  Symbols:
    an int below 256 (literal), EOB, ("match", length, distance), and for malformed streams
    ("code", "ll" | "d", symbol) -- that symbol's Huffman code alone -- and ("bits", value, n)."""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.stored_header_bitpos = []                 # bit position of every stored block's header
        self.hclen = None

    @property
    def pos(self) -> int:
        return len(self.out)

    def stored(self, data: bytes, last: bool = False, nlen: int | None = None) -> "Deflate":
        self.stored_header_bitpos.append(self.w.bitpos)
        self.w.bits(int(last), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        for v in data:
            self.w.bits(v, 8)
        self.out += data
        return self

    def _symbols(self, symbols, ll, d) -> None:
        w = self.w
        for s in symbols:
            if isinstance(s, int):
                w.code(*ll[s])
                if s < 256:
                    self.out.append(s)
            elif s[0] == "match":
                _, length, dist = s
                lc, dc = _len_code(length), _dist_code(dist)
                w.code(*ll[257 + lc])
                w.bits(length - LEN_BASE[lc], LEN_EXTRA[lc])
                w.code(*d[dc])
                w.bits(dist - DIST_BASE[dc], DIST_EXTRA[dc])
                if dist <= len(self.out):              # (a distance beyond the start copies nothing)
                    for _ in range(length):
                        self.out.append(self.out[-dist])
            elif s[0] == "code":
                w.code(*(ll if s[1] == "ll" else d)[s[2]])
            else:
                w.bits(s[1], s[2])

    def fixed(self, symbols, last: bool = False) -> "Deflate":
        self.w.bits(int(last), 1)
        self.w.bits(1, 2)
        self._symbols(symbols, canonical(FIXED_LL), canonical(FIXED_D))
        return self

    def dynamic(self, ll_lengths, d_lengths, symbols, last: bool = False, cl_symbols=None, cl_lengths=None,
                hclen: int | None = None, check: bool = True) -> "Deflate":
        """HLIT = len(ll_lengths), HDIST = len(d_lengths); ``cl_symbols`` is the sequence of
        code-length symbols (sym, extra) written for them, as given (cl_plain when None)."""
        if cl_symbols is None:
            cl_symbols = cl_plain(list(ll_lengths) + list(d_lengths))
        if cl_lengths is None:
            cl_lengths = cl_complete(cl_symbols)
        if check:
            assert expand(cl_symbols) == list(ll_lengths) + list(d_lengths)
            assert kraft(cl_lengths) == 1
        if hclen is None:
            hclen = max(4, 1 + max(k for k in range(19) if cl_lengths[CL_ORDER[k]]))
        self.hclen = hclen
        w = self.w
        w.bits(int(last), 1)
        w.bits(2, 2)
        w.bits(len(ll_lengths) - 257, 5)
        w.bits(len(d_lengths) - 1, 5)
        w.bits(hclen - 4, 4)
        for k in range(hclen):
            w.bits(cl_lengths[CL_ORDER[k]], 3)
        clc = canonical(cl_lengths)
        for s, e in cl_symbols:
            w.code(*clc[s])
            if s >= 16:
                w.bits(e, {16: 2, 17: 3, 18: 7}[s])
        self._symbols(symbols, canonical(ll_lengths), canonical(d_lengths))
        return self

    def bytes(self) -> bytes:
        return self.w.bytes()


def zlib_wrap(deflate: bytes, data: bytes, cinfo: int = 7, flevel: int = 2, fdict: bool = False, cm: int = 8,
              bad_check: bool = False, adler: int | None = None, adler_len: int = 4, tail: bytes = b"") -> bytes:
    """RFC 1950 around a deflate stream: the Adler-32 of the intended bytes unless overridden,
    cut to ``adler_len`` bytes, then ``tail``."""
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (int(fdict) << 5)
    flg |= (31 - ((cmf << 8) | flg) % 31) % 31
    if bad_check:
        flg ^= 1
    a = zlib.adler32(data) if adler is None else adler
    return bytes([cmf, flg]) + (b"\0\0\0\1" if fdict else b"") + deflate + struct.pack(">I", a & 0xffffffff)[:adler_len] + tail


def png(w: int, h: int, ch: int, z: bytes, idat_split=None) -> bytes:
    """An 8-bit PNG whose IDAT payload is ``z``, cut into chunks of the sizes in ``idat_split``
    (zeros allowed; what is left goes into one more chunk)."""
    out = b"\x89PNG\r\n\x1a\n" + png_encode.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[ch], 0, 0, 0))
    at = 0
    for n in ([len(z)] if idat_split is None else idat_split):
        out += png_encode.chunk(b"IDAT", z[at:at + n])
        at += n
    if at < len(z):
        out += png_encode.chunk(b"IDAT", z[at:])
    return out + png_encode.chunk(b"IEND", b"")


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img: np.ndarray, ch: int, filters) -> bytes:
    """PNG §9 scanlines of img [h][w*ch] (uint8) with filter type filters[y % len]."""
    h, rb = img.shape
    out = bytearray()
    prev = np.zeros(rb, np.int64)
    z = np.zeros(ch, np.int64)
    for y in range(h):
        cur = img[y].astype(np.int64)
        ft = filters[y % len(filters)]
        left = np.concatenate([z, cur[:-ch]])
        ul = np.concatenate([z, prev[:-ch]])
        pred = (np.zeros(rb, np.int64), left, prev, (left + prev) >> 1, _paeth(left, prev, ul))[ft]
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def unfilter(raw: bytes, w: int, h: int, ch: int) -> np.ndarray:
    """PNG §9 reconstruction of scanlines, byte by byte as the specification states it."""
    rb = w * ch
    out = np.zeros((h, rb), np.uint8)
    prev = [0] * rb
    for y in range(h):
        ft = raw[y * (rb + 1)]
        s = raw[y * (rb + 1) + 1:(y + 1) * (rb + 1)]
        cur = [0] * rb
        for x in range(rb):
            a = cur[x - ch] if x >= ch else 0
            b = prev[x]
            c = prev[x - ch] if x >= ch else 0
            if ft == 0:
                p = 0
            elif ft == 1:
                p = a
            elif ft == 2:
                p = b
            elif ft == 3:
                p = (a + b) >> 1
            else:
                q = a + b - c
                pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[x] = (s[x] + p) & 255
        out[y] = cur
        prev = cur
    return out


@dataclass(frozen=True)
class Case:
    name: str
    w: int
    h: int
    ch: int
    raw: bytes | None            # the filtered scanlines it must inflate to (None: malformed before any)
    z: bytes                     # the zlib stream
    status: int                  # OK or the SLG_PNG_E_* it must come back with
    path: str                    # the kernel path / exit it exists for
    tags: frozenset
    image: np.ndarray | None = None   # [h][w*ch], valid (and lenient) cases
    lenient: bool = False        # zlib refuses it for an incomplete set only: status != 0 or output == image
    idat_split: tuple | None = None
    unused: bytes = b""          # what zlib's decompressobj leaves in unused_data
    cpu: str = "ok"              # what zlib says: ok | error (zlib.error) | length (other size) | check | none
    complete_sets: tuple = ()    # code-length lists stated complete (Kraft sum 1)
    marks: tuple = ()            # ring cases: (output position, symbol) of the symbols under test, then
                                 # ("waiting", pos - flushed) of the copies that triggered the first flushes

    @property
    def n_out(self) -> int:
        return self.h * (1 + self.w * self.ch)

    def png(self) -> bytes:
        return png(self.w, self.h, self.ch, self.z, self.idat_split)


def _row_case(name, d: Deflate, path, tags, status=OK, cpu="ok", lenient=False, sets=(), idat_split=None, unused=b"",
              extra=0, **zkw) -> Case:
    """The stream's intended bytes as one gray scanline (its first byte, 0, is the filter type);
    ``extra``: the image is that many bytes shorter (< 0: longer) than what the stream inflates to."""
    raw = bytes(d.out)
    assert raw and raw[0] == 0, name
    w = len(raw) - 1 - extra
    assert 1 <= w <= MAX_ROW, (name, w)
    image = np.frombuffer(raw[1:], np.uint8).reshape(1, -1).copy() if status == OK or lenient else None
    return Case(name, w, 1, 1, raw, zlib_wrap(d.bytes(), raw, **zkw), status, path, frozenset(tags), image, lenient,
                idat_split, unused, cpu, tuple(tuple(s) for s in sets))


def _image_case(name, img, ch, z_of_raw, path, tags, filters=(0,), status=OK, cpu="ok", poke=None) -> Case:
    """A case made from the image: its scanlines filtered, compressed by ``z_of_raw`` (raw -> zlib
    stream); ``poke`` = (row, value) overwrites one filter byte first."""
    h, rb = img.shape
    raw = bytearray(filter_rows(img, ch, filters))
    if poke:
        raw[poke[0] * (rb + 1)] = poke[1]
    raw = bytes(raw)
    return Case(name, rb // ch, h, ch, raw, z_of_raw(raw), status, path, frozenset(tags),
                img if status == OK else None, cpu=cpu)


def _real(level=6, wbits=15, flush_rows=0):
    def f(raw):
        co = zlib.compressobj(level, zlib.DEFLATED, wbits)
        if not flush_rows:
            return co.compress(raw) + co.flush()
        out = b""
        for k in range(0, len(raw), flush_rows):
            out += co.compress(raw[k:k + flush_rows]) + co.flush(zlib.Z_FULL_FLUSH)
        return out + co.flush()
    return f


class Script:
    """A symbol list under construction that knows the output position after every symbol and
    what the kernel's flush counter (a 2 KB block leaves the ring once 2,048 bytes wait) stands at."""

    def __init__(self, seed: int, alphabet=(0, 1, 2, 3, 4)):
        self.sym = []
        self.pos = 0
        self.flushed = 0
        self.waiting = []                              # pos - flushed after every copy, before its flush
        self.rng = random.Random(seed)
        self.alphabet = alphabet

    def _after(self, copy):
        if copy:
            self.waiting.append(self.pos - self.flushed)
        if self.pos - self.flushed >= FLUSH:
            self.flushed += FLUSH
        assert self.pos - self.flushed < FLUSH

    def lit(self, v=None):
        self.sym.append(self.rng.choice(self.alphabet) if v is None else v)
        self.pos += 1
        self._after(False)
        return self

    def match(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= min(self.pos, 32768), (length, dist, self.pos)
        self.sym.append(("match", length, dist))
        self.pos += length
        self._after(True)
        return self

    def fill_to(self, target):
        """Pseudo-random literals and copies (any length, any distance in the window) up to ``target``."""
        assert target >= self.pos
        while self.pos < target:
            rem = target - self.pos
            if self.pos == 0:
                self.lit(0)
            elif rem < 3 or self.rng.random() < 0.3:
                self.lit()
            else:
                length = min(rem, self.rng.choice((258, 258, self.rng.randint(3, 258))))
                self.match(length, self.rng.randint(1, min(self.pos, 32768)))
        return self


# The literal/length set of the ring cases: literals 0..4 in 3 bits (so one 11-bit literal-run
# lookup yields 3 of them), length code 285 in 3 bits, end-of-block and the other 28 length codes
# share the last quarter.  Every byte is then a valid filter type, wherever a scanline starts.
_RING_LL = table(286, {**{v: 3 for v in range(5)}, 285: 3, **dict(zip(range(256, 285), balanced(29, 2)))})
_ALL_D = balanced(30)
_RING_W, _RING_H = 99, 372                             # 37,200 inflated bytes
_FLUSH_TAGS = ("flush_wait_2048", "flush_wait_2305")


def _ring_case(name, seed, at, event, path, tags, total=_RING_H * (_RING_W + 1), w=_RING_W, ll=_RING_LL) -> Case:
    """An image whose stream first makes a copy end with exactly 2,048 and with 2,048 + 257 bytes
    waiting for their flush, then reaches output position ``at`` by a copy, where ``event(script)``
    places the symbols under test; pseudo-random copies fill the rest."""
    s = Script(seed)
    s.fill_to(FLUSH - 100).match(100, 77)
    assert s.waiting[-1] == FLUSH and s.pos == FLUSH
    s.fill_to(2 * FLUSH - 1).match(258, 1000)
    assert s.waiting[-1] == FLUSH + 257
    s.fill_to(at - 258).match(258, 4001)               # (a copy ends at `at`: what follows starts a lookup)
    assert s.pos == at
    first = len(s.sym) - 1
    event(s)
    marks, p = [], at - 258                            # the copy that ends at `at` and every symbol under test,
                                                       # each with the position it starts at
    for sym in s.sym[first:]:
        marks.append((p, sym))
        p += 1 if isinstance(sym, int) else sym[1]
    waits = tuple(("waiting", n) for n in s.waiting[:s.waiting.index(FLUSH + 257) + 1] if n >= FLUSH)
    s.fill_to(total)
    d = Deflate().dynamic(ll, _ALL_D, s.sym + [EOB], last=True, cl_symbols=cl_rle(ll + _ALL_D))
    raw = bytes(d.out)
    assert len(raw) == total == s.pos
    h = total // (w + 1)
    return Case(name, w, h, 1, raw, zlib_wrap(d.bytes(), raw), OK, path, frozenset(tags) | set(_FLUSH_TAGS),
                unfilter(raw, w, h, 1), complete_sets=(tuple(ll), tuple(_ALL_D)),
                marks=tuple(marks) + waits)


def _valid() -> list:
    C = []
    rng = np.random.default_rng(5)

    # 1. repeat codes across the HLIT boundary -------------------------------------------------
    ll = table(260, {0: 3, 1: 3, 2: 3, 256: 3, 258: 2, 259: 2})        # 258: length 4, 259: length 5
    dl = [2, 2, 2, 2]
    data = [0, 1, 2, 1, 0, 2, ("match", 4, 1), ("match", 5, 3), ("match", 4, 4), ("match", 5, 2), 1, EOB]
    cl = [(3, 0), (3, 0), (3, 0), (18, 127), (18, 104), (3, 0), (0, 0), (2, 0), (16, 2)]   # 16: lengths 259 | 0..3
    C.append(_row_case("repeat16_across_hlit", Deflate().dynamic(ll, dl, data, True, cl),
                       "lens[k < hlit ? k : 288 + k - hlit] with i < hlit < i + rep, v = prev", {"repeat16_cross"},
                       sets=(ll, dl)))
    cl = [(3, 0), (3, 0), (3, 0), (18, 127), (18, 104), (3, 0), (0, 0), (2, 0), (2, 0), (16, 1)]   # 16 at i == hlit
    C.append(_row_case("repeat16_first_after_hlit", Deflate().dynamic(ll, dl, data, True, cl),
                       "code 16 at i == hlit: prev carried from the last literal/length length", {"repeat16_at_boundary"},
                       sets=(ll, dl)))
    ll = table(262, {0: 2, 1: 2, 256: 2, 257: 2})
    dl = [0, 0, 0, 1, 1]                                                # distance 4, 5..6
    data = [0, 1, 1, 0, 1, 0, 0, ("match", 3, 4), ("match", 3, 6), 1, ("match", 3, 5), EOB]
    cl = [(2, 0), (2, 0), (18, 127), (18, 105), (2, 0), (2, 0), (17, 4), (1, 0), (1, 0)]   # 17: 258..261 | 0..2
    C.append(_row_case("repeat17_across_hlit", Deflate().dynamic(ll, dl, data, True, cl),
                       "code 17 with i < hlit < i + rep", {"repeat17_cross"}, sets=(ll, dl)))
    ll = table(270, {0: 2, 1: 2, 256: 2, 257: 2})
    dl = [0] * 10 + [1, 1]                                              # distance 33..48, 49..64
    data = [0] + [int(v) for v in rng.integers(0, 2, 70)] + [("match", 3, 33), ("match", 3, 48), ("match", 3, 49),
                                                              ("match", 3, 64), 1, EOB]
    cl = [(2, 0), (2, 0), (18, 127), (18, 105), (2, 0), (2, 0), (18, 11), (1, 0), (1, 0)]  # 18: 258..269 | 0..9
    C.append(_row_case("repeat18_across_hlit", Deflate().dynamic(ll, dl, data, True, cl),
                       "code 18 with i < hlit < i + rep", {"repeat18_cross"}, sets=(ll, dl)))

    # 2./3. one distance code of one bit; no distance code ------------------------------------------
    ll = table(259, {0: 2, 1: 3, 2: 3, 256: 2, 257: 3, 258: 3})
    data = [0, 1, 2, ("match", 3, 3), 2, 1, 0, ("match", 4, 3), ("match", 3, 3), 1, EOB]
    C.append(_row_case("one_distance_code", Deflate().dynamic(ll, [0, 0, 1], data, True),
                       "build() of an incomplete distance set: one 1-bit code", {"one_dist_code"}, sets=(ll,)))
    ll = table(257, {0: 2, 7: 2, 200: 2, 256: 2})
    C.append(_row_case("no_distance_code", Deflate().dynamic(ll, [0], [0, 7, 200, 200, 7, 0, 7, EOB], True),
                       "HDIST = 1 with length 0: build() of an empty set (literal-only block)", {"no_dist_code"},
                       sets=(ll,)))

    # 4. a set holding only end-of-block, then an unaligned stored block -------------------------------
    d = Deflate().dynamic(table(257, {256: 1}), [0], [EOB], False, [(18, 127), (18, 107), (1, 0), (0, 0)],
                          table(19, {18: 1, 1: 2, 0: 2}))
    assert (d.w.bitpos + 3) % 8 != 0
    d.stored(bytes([0, 9, 8, 7, 250, 251]), True)
    C.append(_row_case("eob_only_set_then_stored", d, "a literal/length set of one 1-bit code; stored-block byte alignment",
                       {"eob_only_set", "stored_unaligned"}))

    # 5. the 15-bit ladder: 1, 2, ..., 14, 15, 15 ------------------------------------------------------
    ll = table(257, {**{v: v + 1 for v in range(13)}, 256: 14, 13: 15, 14: 15})
    data = [0, 13, 14, 10, 0, 1, 12, 14, 13, 11, 10, 2, 3, 4, 5, 6, 7, 8, 9, 13, EOB]
    d = Deflate().dynamic(ll, [0], data, True, cl_rle(ll + [0]))
    assert d.hclen == 19 and sorted(l for l in ll if l) == list(range(1, 15)) + [15, 15]
    C.append(_row_case("ladder_15_literals", d, "decode_slow: 11..15-bit literal codes (past kFastBits = 10); HCLEN = 19",
                       {"long_codes", "hclen_19"}, sets=(ll,)))
    dl = list(range(1, 15)) + [15, 15]                                  # distance codes 0..15
    ll = table(259, {0: 2, 1: 2, 256: 3, 257: 3, 258: 2})
    data = [0] + [int(v) for v in rng.integers(0, 2, 260)] + \
        [("match", 4, 193), ("match", 3, 129), ("match", 4, 256), ("match", 3, 33), ("match", 4, 192), ("match", 3, 1), EOB]
    C.append(_row_case("ladder_15_distances", Deflate().dynamic(ll, dl, data, True, cl_rle(ll + dl)),
                       "decode_slow on the distance table: 11- and 15-bit distance codes", {"long_codes"}, sets=(ll, dl)))

    # 6. maximal sets and the extreme length / distance codes; 10. the ring's ends ---------------------
    ll286 = balanced(286)

    def extremes(s):
        s.match(258, 32768)                            # code 285; distance code 29, all 13 extra bits set
        s.match(257, 1)                                # code 284 with extra 30; distance code 0
        s.match(258, 32768)
    C.append(_ring_case("max_sets_len258_dist32768_at_40000", 21, 40000, extremes,
                        "HLIT = 286, HDIST = 30; length codes 285 and 284 + 30, distance codes 29 + 8191 and 0; "
                        "dist > pos is false for 32,768 at pos 40,000",
                        {"hlit_286_hdist_30", "len258_dist32768", "len284_extra30", "dist_code_0", "far_distance_ok"},
                        total=410 * 100, ll=ll286))
    C.append(_ring_case("ring_copy_258_at_32768_over_end", 22, RING - 4, lambda s: s.match(258, 32768),
                        "copy loop: di wraps at kRing, si = ridx - 32768 + kRing (a)", {"ring_far_copy", "len258_dist32768"}))
    C.append(_ring_case("ring_copy_dist1_over_end", 23, RING - 64, lambda s: s.match(258, 1),
                        "copy loop, i % dist with dist 1, di wraps (b)", {"ring_near_copy"}))
    C.append(_ring_case("ring_copy_dist63_over_end", 24, RING - 30, lambda s: s.match(258, 63),
                        "copy loop, i % dist with dist 63: si and di wrap (b)", {"ring_near_copy"}))
    for back in (1, 2, 3):
        C.append(_ring_case(f"ring_literal_run_at_{RING - back}", 24 + back, RING - back,
                            lambda s: [s.lit() for _ in range(9)],
                            f"literal-run word at ring offset {RING - back}: the 4 slack bytes and the wrapped bytes (c)",
                            {"ring_literal_run"}))
    C.append(_ring_case("ring_copy_ends_at_end", 28, RING, lambda s: [s.lit() for _ in range(4)] and s.match(100, 36000 - 4000),
                        "ridx += len reaches kRing exactly, ridx -= kRing (d)", {"ring_copy_to_end"}))

    # 7. the fewest code-length lengths a block with an end-of-block code can have; HCLEN = 19 is case 5
    ll = table(257, {**{v: 8 for v in range(255)}, 256: 8})
    cl = [(8, 0)] + [(16, 3)] * 41 + [(16, 1), (16, 1), (0, 0), (8, 0), (0, 0)]
    data = [0] + [int(v) for v in rng.integers(0, 255, 40)] + [254, EOB]
    d = Deflate().dynamic(ll, [0], data, True, cl, table(19, {16: 2, 17: 3, 18: 3, 0: 2, 8: 2}))
    assert d.hclen == 5
    C.append(_row_case("hclen_5", d, "HCLEN = 5 (16, 17, 18, 0, 8): cl[] beyond hclen stays 0", {"hclen_min"}, sets=(ll,)))

    # 8. flush markers ---------------------------------------------------------------------------
    seen = set()
    for k in range(8):
        d = Deflate().fixed([0, 65] + [200] * k + [EOB])               # 9-bit literals move the alignment
        d.stored(b"")
        d.fixed([66, 201, ("match", 3, 2), EOB], True)
        seen.add(d.stored_header_bitpos[0] % 8)
        C.append(_row_case(f"sync_flush_at_bit_{d.stored_header_bitpos[0] % 8}", d,
                           "empty stored block (LEN = 0) between compressed blocks: drop = cnt & 7", {"flush_stored_empty"}))
    assert seen == set(range(8))
    d = Deflate().fixed([0, 1, 2, 3, EOB]).fixed([EOB]).fixed([4, ("match", 4, 5), EOB], True)
    C.append(_row_case("partial_flush_empty_fixed", d, "empty fixed block in mid-stream", {"flush_fixed_empty"}))
    img = rng.integers(0, 256, (255, 256), dtype=np.uint8)
    c = _image_case("stored_65535", img, 1, lambda raw: zlib_wrap(Deflate().stored(raw, True).bytes(), raw),
                    "stored block of LEN = 65,535: put() across 31 flushes and the ring's end", {"stored_max"}, (0, 1, 2, 3, 4))
    assert len(c.raw) == 65535
    C.append(c)
    img = (np.add.outer(np.arange(70), np.arange(90)) % 251).astype(np.uint8)
    c = _image_case("full_flush_per_row", img, 1, _real(6, 15, 91), "70 blocks, each followed by an empty stored block",
                    {"flush_per_row"}, (1, 2, 4))
    assert c.z.count(b"\x00\x00\xff\xff") >= 64
    C.append(c)

    # 9. zlib headers ------------------------------------------------------------------------------
    img = (np.add.outer(np.arange(40), 3 * np.arange(50)) % 256).astype(np.uint8)
    for wbits in (9, 12, 15):
        c = _image_case(f"zlib_wbits_{wbits}", img, 1, _real(9, wbits), f"header test: CINFO = {wbits - 8}",
                        {"small_window"} if wbits < 15 else {"window_32k"}, (0, 1, 2, 3, 4))
        assert c.z[0] >> 4 == wbits - 8
        C.append(c)
    for fl in range(4):
        C.append(_row_case(f"zlib_flevel_{fl}", Deflate().fixed([0, 5, 6, ("match", 5, 2), EOB], True),
                           "header test: FLEVEL is not looked at", {"flevel"}, flevel=fl))

    # 11. overlapped copies with distance >= 64 and length > distance ---------------------------------
    for dist in (64, 100):
        lits = [0] + [int(v) for v in rng.integers(0, 256, dist + 5)]
        d = Deflate().fixed(lits + [("match", 258, dist), 3, ("match", 258, dist), EOB], True)
        C.append(_row_case(f"overlap_dist{dist}_len258", d,
                           "copy loop, dist >= 64 < len: a 64-lane step reads what the step before wrote", {"overlap_far"}))

    # 12./13. IDAT layout; bytes behind the Adler-32 ----------------------------------------------------
    base = C[0]
    n = len(base.z)
    for name, split in (("idat_1_byte_chunks", (1,) * n), ("idat_empty_chunks_header_and_trailer_split", (0, 1, 0, n - 3, 0, 2, 0))):
        C.append(Case(name, base.w, base.h, base.ch, base.raw, base.z, OK, "slg_png_zstream: IDAT payloads concatenated",
                      frozenset({"idat_split"}), base.image, idat_split=split))
    C.append(_row_case("bytes_after_adler", Deflate().fixed([0, 5, 6, ("match", 5, 2), EOB], True),
                       "the trailer is read at the next byte boundary; what follows is not looked at", {"trailing_bytes"},
                       tail=b"\x00\xffjunk", unused=b"\x00\xffjunk"))

    # 14. un-filter -----------------------------------------------------------------------------
    for h in (1, 64, 65, 130):
        img = rng.integers(0, 256, (h, 2 * 37), dtype=np.uint8)
        for ft in range(5):
            C.append(_image_case(f"gray_alpha_filter{ft}_h{h}", img, 2, _real(),
                                 "unfilter_frame<2>: bands of 64 rows handed over through lastrow", {"gray_alpha"}, (ft,)))
    img = (np.add.outer(7 * np.arange(65), np.arange(MAX_ROW)) // 5 % 256).astype(np.uint8)
    C.append(_image_case("row_bytes_24576", img[:1], 4, _real(1), "width * channels == kMaxRowBytes", {"row_24576"}, (1,)))
    C.append(_image_case("row_bytes_24576_two_bands", img, 4, _real(1), "lastrow[24575] across the band hand-over",
                         {"row_24576"}, (4, 3)))
    for ch in (2, 4):
        img = rng.integers(0, 256, (70, ch), dtype=np.uint8)
        C.append(_image_case(f"one_pixel_wide_{ch}ch", img, ch, _real(), "rb == BPP: every byte's left neighbour is 0",
                             {"one_pixel_wide"} | ({"gray_alpha"} if ch == 2 else set()), (0, 1, 2, 3, 4)))
    return C


def _bad_header(name, path, tags, **zkw) -> Case:
    d = Deflate().fixed([0, 1, 2, 3, EOB], True)
    return _row_case(name, d, path, set(tags) | {"E_STREAM"}, E_STREAM, "error", **zkw)


def _raw_case(name, d: Deflate, status, path, tags, cpu="error", w=8) -> Case:
    """A malformed stream with no intended output, for a 1-row gray image of ``w`` pixels."""
    return Case(name, w, 1, 1, None, zlib_wrap(d.bytes(), b""), status, path,
                frozenset(tags) | {("", "E_STREAM", "E_SIZE", "E_ADLER", "E_FILTER", "E_UNSUPPORTED")[status]}, cpu=cpu)


def _invalid() -> list:
    C = []
    rng = np.random.default_rng(6)
    hdr = "zlib header test -> E_STREAM"
    C.append(_bad_header("fdict_set", hdr, {"fdict"}, fdict=True))
    C.append(_bad_header("cm_not_8", hdr, {"bad_cm"}, cm=7))
    C.append(_bad_header("cinfo_8", hdr, {"bad_cinfo"}, cinfo=8))
    C.append(_bad_header("fcheck_wrong", hdr, {"bad_fcheck"}, bad_check=True))

    d = Deflate()
    d.w.bits(1, 1)
    d.w.bits(3, 2)
    d.w.bits(0, 13)
    C.append(_raw_case("block_type_3", d, E_STREAM, "type == 3", {"block_type_3"}))
    d = Deflate().stored(bytes(9), True, nlen=0xfff7)                   # ~9 is 0xfff6
    C.append(_raw_case("stored_nlen_mismatch", d, E_STREAM, "stored block: (len ^ 0xffff) != nlen", {"stored_nlen"}))
    d = Deflate().stored(bytes(10), True)
    C.append(_row_case("stored_longer_than_image", d, "stored block: pos + len > n_out -> E_STREAM (not E_SIZE)",
                       {"stored_overrun", "E_STREAM"}, E_STREAM, "length", extra=1))

    ll = table(257, {0: 1, 256: 1})
    for name, hl, hd in (("hlit_287", 287, 1), ("hdist_31", 257, 31)):
        d = Deflate().dynamic(ll + [0] * (hl - 257), [0] * hd, [0, 0, EOB], True, cl_rle(ll + [0] * (hl - 257 + hd)))
        C.append(_raw_case(name, d, E_STREAM, "hlit > 286 || hdist > 30", {name}, w=1))

    # over-subscribed sets: build() false
    d = Deflate().dynamic(ll, [0], [0, 0, EOB], True, cl_plain(ll + [0]), table(19, {0: 1, 1: 1, 2: 1}), check=False)
    C.append(_raw_case("oversubscribed_code_length_set", d, E_STREAM, "build(code-length code) false", {"oversubscribed_cl"}, w=1))
    bad = table(257, {0: 1, 1: 1, 256: 1})
    d = Deflate().dynamic(bad, [0], [0, 0, EOB], True, cl_rle(bad + [0]))
    C.append(_raw_case("oversubscribed_litlen_set", d, E_STREAM, "build(L.lit) false", {"oversubscribed_ll"}, w=1))
    d = Deflate().dynamic(ll, [1, 1, 1], [0, 0, EOB], True, cl_rle(ll + [1, 1, 1]))
    C.append(_raw_case("oversubscribed_distance_set", d, E_STREAM, "build(L.dist) false", {"oversubscribed_d"}, w=1))

    # repeat checks
    d = Deflate().dynamic(ll, [0], [0, 0, EOB], True, [(16, 0)] + cl_plain(ll[3:] + [0]),
                          table(19, {16: 2, 0: 2, 1: 2, 18: 2}), check=False)
    C.append(_raw_case("repeat16_first", d, E_STREAM, "s == 16 with i == 0", {"repeat16_first"}, w=1))
    d = Deflate().dynamic(ll, [0], [0, 0, EOB], True, [(1, 0), (18, 127), (18, 106), (1, 0), (17, 0)], check=False)
    C.append(_raw_case("repeat_past_hlit_hdist", d, E_STREAM, "i + rep > hlit + hdist", {"repeat_overrun"}, w=1))

    # no end-of-block code; this is also all HCLEN = 4 can say (16, 17, 18 and 0 only: every length is 0)
    z = table(257, {})
    d = Deflate().dynamic(z, [0], [], True, [(18, 127), (18, 109)], table(19, {16: 2, 17: 2, 18: 2, 0: 2}))
    assert d.hclen == 4
    C.append(_raw_case("hclen_4_no_end_of_block", d, E_STREAM, "L.lens[256] == 0", {"no_eob", "hclen_4"}, w=1))
    noeob = table(257, {0: 1, 1: 1})
    d = Deflate().dynamic(noeob, [0], [0, 1, 1, 0], True)
    C.append(_raw_case("no_end_of_block_code", d, E_STREAM, "L.lens[256] == 0", {"no_eob"}, w=3))

    # a code that an incomplete set does not have
    ll3 = table(258, {0: 2, 1: 2, 256: 2, 257: 2})
    d = Deflate().dynamic(ll3, [0, 0, 1], [0, 1, 1, ("code", "ll", 257), ("bits", 1, 1), 0, EOB], True)
    C.append(_raw_case("absent_distance_code", d, E_STREAM, "decode(L.dist) < 0: the 1-bit set's other code", {"absent_code"}))
    inc = table(257, {0: 2, 1: 2, 256: 2})
    d = Deflate().dynamic(inc, [0], [0, 1, 1, ("bits", 3, 2), 0, EOB], True)
    C.append(_raw_case("absent_litlen_code", d, E_STREAM, "decode(L.lit) < 0: code 11 of a set holding 00, 01, 10",
                       {"absent_code"}))

    # fixed-block symbols that are no symbols
    for s in (286, 287):
        d = Deflate().fixed([0, 1, 2, ("code", "ll", s), ("code", "d", 0), EOB], True)
        C.append(_raw_case(f"fixed_length_symbol_{s}", d, E_STREAM, "s >= 29", {"fixed_len_286_287"}))
    for s in (30, 31):
        d = Deflate().fixed([0, 1, 2, ("code", "ll", 257), ("code", "d", s), EOB], True)
        C.append(_raw_case(f"fixed_distance_code_{s}", d, E_STREAM, "decode(L.dist) < 0: 30 5-bit codes built, 30 and 31 missing",
                           {"fixed_dist_30_31"}))

    # distance beyond the start
    d = Deflate().fixed([0, ("match", 3, 2), 1, 1, 1, 1, EOB], True)
    C.append(_raw_case("distance_2_at_pos_1", d, E_STREAM, "dist > pos", {"dist_too_far"}))
    d = Deflate().fixed([0] + [int(v) for v in rng.integers(0, 256, 99)] + [("match", 3, 101), EOB], True)
    C.append(_raw_case("distance_101_at_pos_100", d, E_STREAM, "dist > pos (32,768 at 40,000 is the valid twin)",
                       {"dist_too_far"}, w=102))

    # the inflated size
    lits = [0, 3, 1, 4, 1, 5, 2, 6, 5, 3, 5]
    C.append(_row_case("one_byte_short", Deflate().fixed(lits + [EOB], True), "pos != n_out after the last block",
                       {"size_short", "E_SIZE"}, E_SIZE, "length", extra=-1))
    ladder = table(257, {**{v: v + 1 for v in range(13)}, 256: 14, 13: 15, 14: 15})
    d = Deflate().dynamic(ladder, [0], [0, 1, 2, 13, 14, 13, EOB], True, cl_rle(ladder + [0]))
    C.append(_row_case("one_byte_over_by_literal", d, "pos >= n_out in the one-literal path (a 15-bit code: no literal run)",
                       {"size_literal", "E_SIZE"}, E_SIZE, "length", extra=1, sets=(ladder,)))
    small = table(257, {0: 2, 1: 2, 2: 2, 256: 2})
    d = Deflate().dynamic(small, [0], [0, 1, 2, 1, 2, 2, 1, EOB], True)
    C.append(_row_case("one_byte_over_by_literal_run", d, "pos + n4 > n_out in the literal-run path (2-bit codes)",
                       {"size_literal_run", "E_SIZE"}, E_SIZE, "length", extra=1, sets=(small,)))
    d = Deflate().fixed([0, 1, 2, 3, ("match", 10, 3), EOB], True)
    C.append(_row_case("one_byte_over_by_copy", d, "pos + len > n_out", {"size_copy", "E_SIZE"}, E_SIZE, "length", extra=1))

    # truncation: reads past zlen give zero bits, 0000000 is the fixed code of end-of-block
    lits = [0] + [int(v) for v in rng.integers(1, 144, 40)]
    for last, status, end in ((True, E_SIZE, "zeros decode as end-of-block of the last block: pos != n_out"),
                              (False, E_STREAM, "zeros decode as end-of-block, then as a stored block with NLEN == LEN == 0")):
        d = Deflate().fixed(lits + [EOB], last)
        if not last:
            d.fixed([EOB], True)
        c = _row_case(f"truncated_in_block_last{int(last)}", d, "truncated inside a block: " + end,
                      {"truncated_block", ("", "E_STREAM", "E_SIZE")[status]}, status, "error")
        C.append(Case(**{**c.__dict__, "z": c.z[:20]}))
    c = _row_case("truncated_in_trailer", Deflate().fixed(lits + [EOB], True), "at + 4 > zlen",
                  {"truncated_trailer", "E_STREAM"}, E_STREAM, "none", adler_len=2)
    C.append(c)

    # what the un-filter kernel refuses
    d = Deflate().fixed(lits + [EOB], True)
    good = zlib.adler32(bytes(d.out))
    for name, a in (("adler_a_off_by_one", (good & 0xffff0000) | ((good + 1) & 0xffff)), ("adler_b_off_by_one", good + 0x10000)):
        C.append(_row_case(name, Deflate().fixed(lits + [EOB], True), "un-filter: computed Adler-32 != trailer",
                           {"adler", "E_ADLER"}, E_ADLER, "check", adler=a))
    img = rng.integers(0, 256, (130, 21), dtype=np.uint8)
    for row in (0, 63, 64, 129):
        for v in (5, 255):
            C.append(_image_case(f"filter_byte_{v}_row_{row}", img, 1, _real(), "un-filter: ft > 4", {"filter_byte", "E_FILTER"},
                                 (0, 1, 2, 3, 4), E_FILTER, "none", poke=(row, v)))
    img = np.zeros((1, MAX_ROW + 1), np.uint8)
    C.append(_image_case("row_bytes_24577", img, 1, _real(), "width * channels > kMaxRowBytes", {"row_24577", "E_UNSUPPORTED"},
                         (0,), E_UNSUPPORTED, "none"))

    # lenient: sets zlib refuses only for being incomplete; the kernel decodes the codes present
    d = Deflate().dynamic(inc, [0], [0, 1, 1, 0, 1, EOB], True)
    C.append(_row_case("incomplete_litlen_set", d, "build() of an incomplete literal/length set of 3 codes: decodes those present",
                       {"lenient_ll"}, OK, "error", lenient=True))
    ll4 = table(258, {0: 2, 1: 2, 256: 2, 257: 2})
    d = Deflate().dynamic(ll4, [2, 2, 2], [0, 1, 1, 0, ("match", 3, 2), ("match", 3, 3), ("match", 3, 1), EOB], True)
    C.append(_row_case("incomplete_distance_set", d, "build() of an incomplete distance set of 3 codes: decodes those present",
                       {"lenient_d"}, OK, "error", lenient=True, sets=(ll4,)))
    return C


@functools.lru_cache(maxsize=None)
def valid() -> tuple:
    return tuple(_valid())


@functools.lru_cache(maxsize=None)
def invalid() -> tuple:
    """The refused streams and, marked ``lenient``, those the kernel may decode."""
    return tuple(_invalid())


# --- a whole frame written the way a foreign encoder might: for the end-to-end test ---------------

def _rev(code: int, length: int) -> int:
    return int(format(code, f"0{length}b")[::-1], 2)


def crosses_hlit(cl_symbols, hlit: int) -> bool:
    """Whether a repeat code of the sequence starts below ``hlit`` and ends above it."""
    i = 0
    for s, e in cl_symbols:
        n = 1 if s < 16 else (3 + e if s < 18 else 11 + e)
        if s >= 16 and i < hlit < i + n:
            return True
        i += n
    return False


def foreign_frame(img: np.ndarray) -> bytes:
    """zlib stream of a gray image [h][w] (filter type 0) written the way a foreign encoder might:
    one dynamic block and one sync flush (an empty stored block) per scanline, a run of 5 to 259
    equal bytes as two literals and a copy at distance 2 under a distance set of that single
    1-bit code, the code lengths run-length coded with a zero run across the HLIT boundary.  The
    frame's blocks share one Huffman set, so the bits are laid out for all rows at once (NumPy)."""
    h, w = img.shape
    R = w + 1
    raw = np.zeros((h, R), np.uint8)
    raw[:, 1:] = img
    a = raw.reshape(-1)
    start = np.ones(h * R, bool)
    start[1:] = a[1:] != a[:-1]
    start[::R] = True                                  # (a run ends with its row)
    starts = np.flatnonzero(start)
    runs = np.diff(np.append(starts, h * R))
    keep = np.ones(h * R, bool)
    matches = {}                                       # position of the run's second literal -> copy length
    for s0, n in zip(starts[(runs >= 5) & (runs <= 259)].tolist(), runs[(runs >= 5) & (runs <= 259)].tolist()):
        keep[s0 + 2:s0 + n] = False
        matches[s0 + 1] = n - 2
    used = sorted(set(np.unique(a[keep]).tolist()) | {EOB} | {257 + _len_code(m) for m in matches.values()})
    ll = table(286, dict(zip(used, balanced(len(used)))))
    dl = [0, 1]
    cl = cl_rle(ll + dl)
    assert crosses_hlit(cl, 286) and kraft(ll) == 1
    head = Deflate().dynamic(ll, dl, [], False, cl)
    n_head = head.w.bitpos
    head = int.from_bytes(bytes(head.w.out) + bytes([head.w.acc]), "little")
    codes = canonical(ll)
    rev = np.array([_rev(*c) if c else 0 for c in codes], np.int64)
    length = np.array(ll, np.int64)
    pos = np.flatnonzero(keep)
    val, nb = rev[a[pos]], length[a[pos]]
    for p, m in matches.items():                       # the copy's bits behind its literal's
        lc = _len_code(m)
        k = int(np.searchsorted(pos, p))
        field = rev[257 + lc] | ((m - LEN_BASE[lc]) << int(length[257 + lc]))    # + the distance code: one 0 bit
        val[k] |= field << int(nb[k])
        nb[k] += int(length[257 + lc]) + LEN_EXTRA[lc] + 1
    row = pos // R
    sym_bits = np.bincount(row, weights=nb, minlength=h).astype(np.int64)
    body = n_head + sym_bits + int(length[EOB]) + 3    # header, symbols, end-of-block, the stored block's 3 bits
    total = (body + 7) // 8 * 8 + 32                   # ... its padding and LEN / NLEN
    row_at = np.concatenate([[0], np.cumsum(total)]) + 16                       # (the zlib header)
    before = np.cumsum(nb) - nb
    sym_at = row_at[row] + n_head + before - before[np.searchsorted(pos, np.arange(h) * R)][row]
    f_pos, f_val, f_n = [sym_at], [val], [nb]
    for c in range(0, n_head, 24):
        f_pos.append(row_at[:h] + c)
        f_val.append(np.full(h, (head >> c) & 0xffffff, np.int64))
        f_n.append(np.full(h, min(24, n_head - c), np.int64))
    f_pos += [row_at[:h] + n_head + sym_bits, row_at[1:] - 16]
    f_val += [np.full(h, rev[EOB], np.int64), np.full(h, 0xffff, np.int64)]
    end = int(row_at[h])
    f_pos.append(np.array([end, end + 24]))            # the last block: stored, empty, BFINAL
    f_val.append(np.array([1, 0xffff]))
    n_bytes = (end + 40) // 8
    p = np.concatenate(f_pos)
    wide = np.concatenate(f_val) << (p & 7)
    out = np.zeros(n_bytes + 4, np.int64)
    for j in range(4):
        out += np.bincount((p >> 3) + j, weights=(wide >> (8 * j)) & 255, minlength=n_bytes + 4).astype(np.int64)
    z = bytearray(out[:n_bytes].astype(np.uint8).tobytes())
    z[:2] = zlib_wrap(b"", b"")[:2]
    return bytes(z) + struct.pack(">I", zlib.adler32(raw.tobytes()))
