"""Helpers for the -m gpu tests: run the product (HIP path through the C ABI) on numpy data via torch device
memory.  torch is only plumbing here (device buffers + stream)."""
import numpy as np

import helpers as H
import portfft_amd as pf


def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


def make_descriptor(lengths, prec="f32", batch=1, storage=0, placement=1, fwd_strides=None, bwd_strides=None,
                    fwd_distance=None, bwd_distance=None, fwd_offset=0, bwd_offset=0, fwd_scale=1.0, bwd_scale=1.0):
    d = pf.descriptor(lengths, prec)
    d.number_of_transforms = batch
    d.complex_storage = pf.complex_storage(storage)
    d.placement = pf.placement(placement)
    if fwd_strides is not None:
        d.forward_strides = list(fwd_strides)
    if bwd_strides is not None:
        d.backward_strides = list(bwd_strides)
    if fwd_distance is not None:
        d.forward_distance = fwd_distance
    if bwd_distance is not None:
        d.backward_distance = bwd_distance
    d.forward_offset, d.backward_offset = fwd_offset, bwd_offset
    d.forward_scale, d.backward_scale = fwd_scale, bwd_scale
    return d


GUARD = 64  # elements of padding in front of and behind every user buffer (a multiple of 64: the base alignment stays)

# every_transform: the probe check of helpers, here for the GPU tests (it runs on the tensors' device)
check_every_transform = H.check_every_transform


def _guarded(torch, data, count, dtype, guard, pad=H.PADDING_VALUE):
    """an allocation of guard[0] + count + guard[1] elements holding the padding value `pad` (H.POISON: that NaN, by
    bit pattern), `data` (numpy) copied to the front of the user's part; returns (allocation, the user's buffer: a
    contiguous slice of it)"""
    lo, hi = guard
    alloc = H.full_torch(lo + count + hi, pad, dtype, "cuda")
    if data is not None:
        alloc[lo:lo + data.size].copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return alloc, alloc[lo:lo + count]


def _host(t):
    return t.cpu().numpy()


def execute(desc, direction, in_buf, plan=None, guard=GUARD, pad=H.PADDING_VALUE):
    """Execute on the GPU with every user buffer inside a larger allocation: `guard` elements (an int, or (before,
    after)) of padding in front of and behind it, in each plane of SPLIT_COMPLEX data.  After the execute both guards of
    every buffer must be unchanged, bit for bit, and so must the whole input of an out-of-place execute.  in_buf: flat
    complex numpy array laid out as the descriptor's input domain says.  Returns the whole output buffer: one complex
    array, or the (re, im) planes; in place, of max(input, output count) elements.  pad: what the guards and the whole
    output buffer hold before the call (H.PADDING_VALUE, or H.POISON)."""
    torch = torch_mod()
    plan = plan or desc.commit()
    lo, hi = (guard, guard) if isinstance(guard, int) else guard
    n_out = desc.get_output_count(direction)
    split = desc.complex_storage == pf.complex_storage.SPLIT_COMPLEX
    in_place = desc.placement == pf.placement.IN_PLACE
    fn = plan.compute_forward if direction == pf.direction.FORWARD else plan.compute_backward
    in_buf = np.ascontiguousarray(in_buf)
    planes = [in_buf] if not split else [np.ascontiguousarray(in_buf.real), np.ascontiguousarray(in_buf.imag)]
    dtype = torch.from_numpy(planes[0][:0]).dtype
    count = max(in_buf.size, n_out) if in_place else in_buf.size
    ins = [_guarded(torch, p, count, dtype, (lo, hi), pad) for p in planes]
    if in_place:
        outs = ins
        fn(*[b for _, b in ins])
    else:
        outs = [_guarded(torch, None, n_out, dtype, (lo, hi), pad) for _ in planes]
        fn(*([b for _, b in ins] + [b for _, b in outs]))
    plan.wait()
    what = "%s %s" % ("in place" if in_place else "out of place", "split" if split else "interleaved")
    host_out = [_host(a) for a, _ in outs]
    H.check_guards(host_out if split else host_out[0], lo, count if in_place else n_out, pad=pad, what=what + " output")
    if not in_place:
        host_in = [_host(a) for a, _ in ins]
        H.check_guards(host_in if split else host_in[0], lo, count, pad=pad, what=what + " input")
        H.check_unchanged(planes if split else planes[0],
                          [a[lo:lo + count] for a in host_in] if split else host_in[0][lo:lo + count],
                          what=what + ": the input of an out-of-place execute")
    size = count if in_place else n_out
    body = [a[lo:lo + size] for a in host_out]
    return tuple(body) if split else body[0]


def combine(buf, dtype):
    """the complex values of an output buffer returned by execute()"""
    if not isinstance(buf, tuple):
        return buf.astype(dtype, copy=False)
    out = np.empty(buf[0].size, dtype=dtype)
    out.real, out.imag = buf
    return out


def run(desc, direction, in_buf, plan=None, guard=GUARD):
    """Execute on the GPU (see execute(): guards and the input of an out-of-place execute checked).  Returns the flat
    output buffer (numpy) of get_output_count elements; untouched elements keep the padding value, like the reference's
    tests (fft_test_utils.hpp:452)."""
    out = execute(desc, direction, in_buf, plan, guard)
    return combine(out, in_buf.dtype)[:desc.get_output_count(direction)]


def transform_packed(desc, direction, packed, plan=None, guard=GUARD, pad=H.PADDING_VALUE):
    """packed [batch, *dims] data of the input domain -> packed data of the output domain, through the
    descriptor's actual layout (scatter, run, gather).  Every element of the output buffer outside the output domain
    must still hold the padding value afterwards (reference_data_wrangler.hpp:299-320).  pad: the value of the guards, of
    the input buffer outside the scattered domain and of the whole pre-filled output (H.PADDING_VALUE, or H.POISON)."""
    inv = pf.inv(direction)
    dims = desc.lengths
    b = desc.number_of_transforms
    split = desc.complex_storage == pf.complex_storage.SPLIT_COMPLEX
    # (the padding value in both planes of split storage; interleaved elements hold PADDING_VALUE + 0j)
    buf = H.scatter(packed, desc.get_strides(direction), desc.get_distance(direction), desc.get_offset(direction),
                    desc.get_input_count(direction),
                    pad=pad * (1 + 1j) if split and pad is not H.POISON else pad)
    raw = execute(desc, direction, buf, plan, guard, pad)
    idx = H.element_indices(b, dims, desc.get_strides(inv), desc.get_distance(inv), desc.get_offset(inv))
    H.check_write_set(raw, idx, pad=pad, what="output buffer")
    out = combine(raw, buf.dtype)[:desc.get_output_count(direction)]
    return H.gather(out, b, dims, desc.get_strides(inv), desc.get_distance(inv), desc.get_offset(inv)), out


class Guarded:
    """A device buffer of `count` elements inside a larger allocation: `guard` elements (an int, or (before, after)) of
    the padding value `pad` (H.PADDING_VALUE, or H.POISON) in front of and behind it.  `.buf` is the user's buffer (a
    contiguous slice), filled with `fill` (None: the padding value).  check() copies only the two guards to the host."""

    def __init__(self, count, dtype, guard=GUARD, fill=None, pad=H.PADDING_VALUE):
        torch = torch_mod()
        self.lo, self.hi = (guard, guard) if isinstance(guard, int) else guard
        self.count = count
        self.pad = pad
        self.alloc = H.full_torch(self.lo + count + self.hi, pad, dtype, "cuda")
        self.buf = self.alloc[self.lo:self.lo + count]
        if fill is not None:
            self.buf.fill_(fill)

    def check(self, what="buffer"):
        bands = np.concatenate([_host(self.alloc[:self.lo]), _host(self.alloc[self.lo + self.count:])])
        H.check_guards(bands, self.lo, 0, pad=self.pad, what=what)  # (an element after the buffer is named by its distance past the end)


def guarded_like(t, guard=GUARD, pad=H.PADDING_VALUE):
    """a Guarded copy of the device tensor t"""
    g = Guarded(t.numel(), t.dtype, guard, pad=pad)
    g.buf.copy_(t.reshape(-1))
    return g


RANDOM_CHUNK = 1 << 27  # scalars per call of the generator in fill_random / check_random


def _random_chunks(t):
    torch = torch_mod()
    flat = torch.view_as_real(t).reshape(-1) if t.is_complex() else t.reshape(-1)
    for c, c0 in enumerate(range(0, flat.numel(), RANDOM_CHUNK)):
        yield c, flat[c0:c0 + RANDOM_CHUNK], c0


def fill_random(t, seed):
    """uniform [-1, 1) scalars into every element of the device tensor t, generated on the device chunk by chunk (one
    seed per chunk), so that check_random can compare against the generator without a second buffer of t's size"""
    torch = torch_mod()
    g = torch.Generator(device="cuda")
    for c, part, _ in _random_chunks(t):
        g.manual_seed(seed * 1000003 + c)
        if part.dtype == torch.float16:
            part.copy_(torch.rand(part.numel(), dtype=torch.float32, device="cuda", generator=g).mul_(2).sub_(1))
        else:
            torch.rand(part.numel(), dtype=part.dtype, device="cuda", generator=g, out=part).mul_(2).sub_(1)


def check_random(t, seed, what="input"):
    """t still holds what fill_random(t, seed) wrote, bit for bit"""
    torch = torch_mod()
    g = torch.Generator(device="cuda")
    for c, part, c0 in _random_chunks(t):
        g.manual_seed(seed * 1000003 + c)
        if part.dtype == torch.float16:
            want = torch.rand(part.numel(), dtype=torch.float32, device="cuda", generator=g).mul_(2).sub_(1).to(torch.float16)
        else:
            want = torch.rand(part.numel(), dtype=part.dtype, device="cuda", generator=g).mul_(2).sub_(1)
        H.check_same_bits(part, want, what="%s (scalars from %d)" % (what, c0))
        del want
