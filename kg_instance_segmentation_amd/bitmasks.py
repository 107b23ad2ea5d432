"""Bit-packed instance masks (include/kgnet_hip.h "bit-mask layout"): one bit per pixel in 64-bit words.

Row y of an h x w mask takes wpr = ceil(w / 64) words, bit b of word k of that row is pixel (y, 64 k + b), bits at x >= w are zero, and a
mask occupies ld_words = round_up(h * wpr, 2) words (the padding word is zero), so every mask of a [n, ld_words] buffer is 16-byte
aligned.  A 512 x 512 mask is 32 KB: 8x less than bytes, 32x less than the float32 arrays the reference returns.

pack_host / unpack_host are pure NumPy (no GPU, no library); BitMasks holds the words on the device."""
import numpy as np


def words_per_row(w):
    return (int(w) + 63) // 64


def ld_words(h, w):
    """Words one h x w mask occupies (== kg_mask_bits_ld)."""
    return (int(h) * words_per_row(w) + 1) // 2 * 2


def pack_host(masks):
    """[n, h, w] array (any non-zero value is foreground) -> uint64 words [n, ld_words(h, w)]."""
    m = np.asarray(masks)
    if m.ndim != 3:
        raise ValueError("pack_host: masks must be [n, h, w]")
    n, h, w = m.shape
    wpr = words_per_row(w)
    bits = np.zeros((n, h, wpr * 64), np.uint8)
    bits[:, :, :w] = m != 0
    by = np.packbits(bits, axis=-1, bitorder="little").reshape(n, h * wpr * 8)
    out = np.zeros((n, ld_words(h, w)), "<u8")
    out[:, :h * wpr] = by.view("<u8")
    return out.astype(np.uint64, copy=False)


def unpack_host(words, h, w):
    """uint64 words [n, ld_words(h, w)] -> uint8 [n, h, w] of 0 / 1."""
    wd = np.ascontiguousarray(np.asarray(words).astype("<u8", copy=False))
    n, wpr = wd.shape[0], words_per_row(w)
    if wd.ndim != 2 or wd.shape[1] < h * wpr:
        raise ValueError("unpack_host: words must be [n, >= h * ceil(w / 64)]")
    by = np.ascontiguousarray(wd[:, :h * wpr]).view(np.uint8)
    return np.ascontiguousarray(np.unpackbits(by, axis=-1, bitorder="little").reshape(n, h, wpr * 64)[:, :, :w])


class BitMasks:
    """n masks of h x w pixels as device words: `words` is an int64 tensor [n, ld_words(h, w)] (the bit pattern of the uint64 words)."""
    __slots__ = ("words", "h", "w")

    def __init__(self, words, h, w):
        if words.dim() != 2 or words.shape[1] != ld_words(h, w) or words.element_size() != 8:
            raise ValueError(f"BitMasks: words must be 64-bit [n, {ld_words(h, w)}] for {h} x {w} masks")
        self.words, self.h, self.w = words, int(h), int(w)

    def __len__(self):
        return self.words.shape[0]

    @property
    def device(self):
        return self.words.device

    @property
    def shape(self):
        return (len(self), self.h, self.w)

    @property
    def nbytes(self):
        return self.words.numel() * 8

    def __getitem__(self, idx):
        """Rows by slice or by an index array (NumPy, list or tensor)."""
        import torch
        if isinstance(idx, slice):
            return BitMasks(self.words[idx], self.h, self.w)
        if not torch.is_tensor(idx):
            idx = torch.from_numpy(np.asarray(idx, np.int64).reshape(-1))
        return BitMasks(self.words[idx.to(self.words.device)], self.h, self.w)

    @staticmethod
    def empty(h, w, device, n=0):
        import torch
        return BitMasks(torch.empty(n, ld_words(h, w), dtype=torch.int64, device=device), h, w)

    @staticmethod
    def cat(parts):
        import torch
        h, w = parts[0].h, parts[0].w
        if any((p.h, p.w) != (h, w) for p in parts):
            raise ValueError("BitMasks.cat: masks of different sizes")
        return parts[0] if len(parts) == 1 else BitMasks(torch.cat([p.words for p in parts]), h, w)

    @staticmethod
    def from_words(words, h, w, device):
        """uint64 host words [n, ld_words] (pack_host's output) -> BitMasks on `device`: only the words are uploaded."""
        import torch
        from . import ops
        wd = np.ascontiguousarray(np.asarray(words, np.uint64)).view(np.int64)
        t = ops.h2d(wd, device) if wd.size else torch.empty(wd.shape, dtype=torch.int64, device=device)
        return BitMasks(t, h, w)

    @staticmethod
    def from_dense(masks, device=None):
        """[n, h, w] NumPy array or tensor (any non-zero value is foreground).  NumPy input is packed on the host and only the words are
        uploaded; a tensor is packed on the device by kg_mask_pack_bits.  Both give the same words."""
        import torch
        from . import _lib
        from ._lib import ptr, stream_ptr, c_long
        if isinstance(masks, BitMasks):
            return masks
        if not torch.is_tensor(masks):
            m = np.asarray(masks)
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            return BitMasks.from_words(pack_host(m), m.shape[1], m.shape[2], dev)
        dev = masks.device if device is None else torch.device(device)
        if dev.type != "cuda":
            raise _lib.KGLibraryError("BitMasks.from_dense (MI355X build) needs a GPU device")
        if masks.dim() != 3:
            raise ValueError("from_dense: masks must be [n, h, w]")
        t = masks.to(dev)
        if t.dtype not in (torch.uint8, torch.float32):
            t = (t != 0).to(torch.uint8)
        t = t.contiguous()
        n, h, w = t.shape
        out = BitMasks.empty(h, w, dev, n)
        if n:
            with torch.cuda.device(dev):
                _lib.call("kg_mask_pack_bits", ptr(t), 1 if t.dtype == torch.float32 else 0, n, h, w, ptr(out.words), c_long(ld_words(h, w)),
                          stream_ptr())
        return out

    def _unpack(self, dtype):
        import torch
        from . import _lib
        from ._lib import ptr, stream_ptr, c_long
        wd = self.words.contiguous()
        out = torch.empty(len(self), self.h, self.w, dtype=dtype, device=wd.device)
        if len(self):
            with torch.cuda.device(wd.device):
                _lib.call("kg_mask_unpack_bits", ptr(wd), c_long(wd.shape[1]), len(self), self.h, self.w, ptr(out), 1 if dtype == torch.uint8 else 0,
                          stream_ptr())
        return out

    def to_u8(self):
        """Device uint8 tensor [n, h, w] of 0 / 1 (what predict(device_u8=True) returns)."""
        import torch
        return self._unpack(torch.uint8)

    def to_f32(self):
        import torch
        return self._unpack(torch.float32)

    def words_cpu(self):
        """uint64 host array [n, ld_words]."""
        return self.words.contiguous().cpu().numpy().view(np.uint64)

    def numpy(self):
        """float32 host array [n, h, w] in {0, 1}: exactly what predict() returns.  Only the words cross to the host."""
        return unpack_host(self.words_cpu(), self.h, self.w).astype(np.float32)
