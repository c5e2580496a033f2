"""Fenced buffers (TEST INFRASTRUCTURE ONLY): one flat uint8 allocation = front guard, n slots `stride` bytes apart, back guard,
all of it filled with seeded pseudo-random bytes.  A kernel that stores outside a slot's payload changes a guard or gap byte; one
that loads outside it gives a result that depends on the fill seed.  Neither can leave the allocation: every guard is at least
GUARD_MIN bytes and at least two row pitches, far more than the largest piece any kernel moves (the wide decoder's 1 KB runs).

Works on any torch device ("cpu" for the helper's own tests)."""
import numpy as np

import crtref as R

GUARD_MIN = 4096
ALIGN = 256                      # torch allocations start on 256-byte boundaries (or better); base_off counts from there


def guard_bytes(pitch):
    """bytes of each guard for rows `pitch` bytes apart: >= GUARD_MIN and >= two pitches, a multiple of ALIGN"""
    g = max(GUARD_MIN, 2 * int(pitch))
    return (g + ALIGN - 1) // ALIGN * ALIGN


class Fenced:
    """n slots of `payload` bytes, `stride` bytes apart, the first one guard + base_off bytes into the allocation."""

    def __init__(self, n, payload, stride=None, base_off=0, pitch=0, device="cpu", name="buffer"):
        import torch
        stride = payload if stride is None else int(stride)
        if n < 1 or payload < 1 or stride < payload or base_off < 0 or base_off >= ALIGN:
            raise ValueError("Fenced(%s): n %d payload %d stride %d base_off %d" % (name, n, payload, stride, base_off))
        self.n, self.payload, self.stride, self.base_off, self.name = n, int(payload), stride, int(base_off), name
        self.guard = guard_bytes(pitch)
        self.start = self.guard + self.base_off                     # first payload byte
        self.end = self.start + (n - 1) * stride + self.payload     # one past the last payload byte
        self.total = self.start + n * stride + self.guard
        self.raw = torch.zeros(self.total, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % ALIGN == 0 or device == "cpu", "allocation of %s is not %d-byte aligned" % (name, ALIGN)

    # ---- filling ------------------------------------------------------------------------------------------------------------
    def prefill(self, seed, contents=None):
        """Fill the WHOLE allocation with lcg_bytes(seed), then put `contents` ([n, payload] uint8-viewable, or None: the payloads
        keep the random fill) into the payloads.  Returns the host copy of what the allocation now holds."""
        import torch
        host = R.lcg_bytes(self.total, seed)
        if contents is not None:
            c = np.ascontiguousarray(contents).view(np.uint8).reshape(self.n, self.payload)
            for k in range(self.n):
                host[self.start + k * self.stride:self.start + k * self.stride + self.payload] = c[k]
        self.raw.copy_(torch.from_numpy(host))
        return host

    # ---- views ---------------------------------------------------------------------------------------------------------------
    def view(self, shape, dtype=None):
        """as_strided view [n, *shape] of the payloads (shape: the per-slot dimensions, contiguous inside a slot)"""
        import torch
        dtype = dtype or torch.uint8
        es = torch.empty(0, dtype=dtype).element_size()
        count = int(np.prod(shape))
        if count * es != self.payload:
            raise ValueError("%s: view %r of %d-byte elements is not the %d-byte payload" % (self.name, shape, es, self.payload))
        if self.start % es or self.stride % es:
            raise ValueError("%s: a %d-byte element view needs base and stride on that grid (pass pointers instead)" % (self.name, es))
        typed = self.raw.view(dtype) if es > 1 else self.raw
        inner, acc = [], 1
        for d in reversed(shape):
            inner.insert(0, acc)
            acc *= int(d)
        return torch.as_strided(typed, (self.n,) + tuple(int(d) for d in shape), (self.stride // es,) + tuple(inner), self.start // es)

    def ptr(self):
        return self.raw.data_ptr() + self.start

    def host(self):
        return self.raw.cpu().numpy()

    def payloads(self, host=None):
        """[n, payload] uint8 copy of the payloads (of `host`, a host copy of the allocation, or of the buffer as it stands)"""
        host = self.host() if host is None else host
        return np.stack([host[self.start + k * self.stride:self.start + k * self.stride + self.payload] for k in range(self.n)])

    # ---- the check -----------------------------------------------------------------------------------------------------------
    def outside_mask(self):
        m = np.ones(self.total, dtype=bool)
        for k in range(self.n):
            m[self.start + k * self.stride:self.start + k * self.stride + self.payload] = False
        return m

    def locate(self, off):
        """(region, slot, distance): where byte `off` of the allocation lies relative to the payloads -- region "front guard" /
        "gap" / "back guard" / "payload"; slot = the nearest payload's; distance to the nearest payload edge: -d = d bytes in front of
        slot's first byte, +d = d bytes behind its last byte (1 = the byte right behind it)"""
        if off < self.start:
            return "front guard", 0, off - self.start
        k = min((off - self.start) // self.stride, self.n - 1)
        rel = off - (self.start + k * self.stride)
        if rel < self.payload:
            return "payload", k, 0
        behind = rel - self.payload + 1
        if k == self.n - 1:
            return ("gap" if rel < self.stride else "back guard"), k, behind
        ahead = self.stride - rel                                  # bytes to the next slot's first byte
        return ("gap", k, behind) if behind <= ahead else ("gap", k + 1, -ahead)

    def first_change(self, prefill, now=None):
        """None, or (offset, region, slot, distance, was, is) of the first byte outside the payloads that differs from `prefill`"""
        now = self.host() if now is None else now
        bad = np.flatnonzero((now != prefill) & self.outside_mask())
        if bad.size == 0:
            return None
        off = int(bad[0])
        region, slot, dist = self.locate(off)
        return off, region, slot, dist, int(prefill[off]), int(now[off]), int(bad.size)

    def assert_fence_intact(self, prefill, now=None):
        ch = self.first_change(prefill, now)
        if ch is not None:
            off, region, slot, dist, was, is_, count = ch
            raise AssertionError("%s: %d byte(s) outside the payloads changed; first at offset %d of the allocation, in the %s, "
                                 "%+d bytes from the nearest payload edge (slot %d): 0x%02x -> 0x%02x"
                                 % (self.name, count, off, region, dist, slot, was, is_))

    def assert_unchanged(self, prefill, now=None):
        """read-only buffers: payloads included, the whole allocation is byte-identical"""
        now = self.host() if now is None else now
        self.assert_fence_intact(prefill, now)
        bad = np.flatnonzero(now != prefill)
        assert bad.size == 0, "%s: read-only payload changed, first at offset %d of the allocation" % (self.name, int(bad[0]))
