"""Host-side mirror of portfft::descriptor / portfft::committed_descriptor (names, fields, argument meaning and
error behaviour follow the reference so that tests read like the reference's own tests).

Reference: /root/reference/src/portfft/descriptor.hpp:43-271, committed_descriptor.hpp:58-310, enums.hpp:25-56,
common/exceptions.hpp:32-77.
"""
import copy as _copy
import ctypes as C
import enum

from . import _lib
from ._lib import lib


# ---- enums (enums.hpp:25-56) ----------------------------------------------------------------------------------
class domain(enum.IntEnum):
    REAL = 0
    COMPLEX = 1


class complex_storage(enum.IntEnum):
    INTERLEAVED_COMPLEX = 0
    SPLIT_COMPLEX = 1


class placement(enum.IntEnum):
    IN_PLACE = 0
    OUT_OF_PLACE = 1


class direction(enum.IntEnum):
    FORWARD = 0
    BACKWARD = 1


class layout(enum.IntEnum):
    PACKED = 0
    UNPACKED = 1
    BATCH_INTERLEAVED = 2


def inv(d):
    """enums.hpp:38: the opposite direction."""
    return direction.BACKWARD if d == direction.FORWARD else direction.FORWARD


# ---- exceptions (common/exceptions.hpp:32-77) -----------------------------------------------------------------
class base_error(RuntimeError):
    pass


class internal_error(base_error):
    pass


class invalid_configuration(base_error):
    pass


class unsupported_configuration(base_error):
    pass


class out_of_local_memory_error(unsupported_configuration):
    pass


class hip_error(base_error):
    pass


_STATUS_TO_EXC = {1: invalid_configuration, 2: unsupported_configuration, 3: out_of_local_memory_error,
                  4: internal_error, 5: hip_error}


def _check(status):
    if status != 0:
        raise _STATUS_TO_EXC.get(status, internal_error)(lib.pfft_last_error().decode())


def version():
    return lib.pfft_version().decode()


_SCALAR_NAMES = {0: "f32", 1: "f64", 2: "f16"}


def _precision_code(p):
    """0 fp32, 1 fp64, 2 fp16 storage (IEEE binary16 in memory, computed in fp32: 1-D packed transforms only)"""
    s = str(p).lower()
    if p in (0, "f32") or "float32" in s or "complex64" in s or s in ("float", "single"):
        return 0
    if p in (1, "f64") or "float64" in s or "complex128" in s or s in ("double",):
        return 1
    if p in (2, "f16") or "float16" in s or "complex32" in s or s in ("half",):
        return 2
    raise invalid_configuration("unknown precision %r" % (p,))


class descriptor:
    """portfft::descriptor<Scalar, Domain> (descriptor.hpp:43-271): a plain parameter bag with the same fields."""

    def __init__(self, lengths, scalar="f32", dom=domain.COMPLEX):
        self.scalar = _SCALAR_NAMES[_precision_code(scalar)]
        self.domain = domain(dom)
        self.lengths = [int(x) for x in lengths]
        self.forward_scale = 1.0
        self.backward_scale = 1.0
        self.number_of_transforms = 1
        self.complex_storage = complex_storage.INTERLEAVED_COMPLEX
        self.placement = placement.OUT_OF_PLACE
        # detail::get_default_strides (utils.hpp:190-201)
        strides, total = [0] * len(self.lengths), 1
        for i in reversed(range(len(self.lengths))):
            strides[i] = total
            total *= self.lengths[i]
        self.forward_strides = list(strides)
        self.backward_strides = list(strides)
        self.forward_distance = total
        self.backward_distance = total
        self.forward_offset = 0
        self.backward_offset = 0

    # -- C view ------------------------------------------------------------------------------------------------
    def _c(self):
        d = _lib.pfft_desc_t()
        if len(self.lengths) > _lib.MAX_RANK:
            raise unsupported_configuration("At most %d dimensions are supported" % _lib.MAX_RANK)
        d.precision = _precision_code(self.scalar)
        d.domain = int(self.domain)
        d.rank = len(self.lengths)
        d.complex_storage = int(self.complex_storage)
        d.placement = int(self.placement)
        d.n_forward_strides = len(self.forward_strides)
        d.n_backward_strides = len(self.backward_strides)
        for i, v in enumerate(self.lengths):
            d.lengths[i] = v
        for i, v in enumerate(self.forward_strides[:_lib.MAX_RANK]):
            d.forward_strides[i] = v
        for i, v in enumerate(self.backward_strides[:_lib.MAX_RANK]):
            d.backward_strides[i] = v
        d.forward_distance = self.forward_distance
        d.backward_distance = self.backward_distance
        d.forward_offset = self.forward_offset
        d.backward_offset = self.backward_offset
        d.number_of_transforms = self.number_of_transforms
        d.forward_scale = self.forward_scale
        d.backward_scale = self.backward_scale
        return d

    # -- getters (descriptor.hpp:161-260) --------------------------------------------------------------------
    def get_flattened_length(self):
        return int(lib.pfft_desc_flattened_length(C.byref(self._c())))

    def get_input_count(self, dir):
        return int(lib.pfft_desc_input_count(C.byref(self._c()), int(dir)))

    def get_output_count(self, dir):
        return int(lib.pfft_desc_output_count(C.byref(self._c()), int(dir)))

    def get_strides(self, dir):
        return self.forward_strides if dir == direction.FORWARD else self.backward_strides

    def get_distance(self, dir):
        return self.forward_distance if dir == direction.FORWARD else self.backward_distance

    def get_offset(self, dir):
        return self.forward_offset if dir == direction.FORWARD else self.backward_offset

    def get_scale(self, dir):
        return self.forward_scale if dir == direction.FORWARD else self.backward_scale

    def get_layout(self, dir):
        """detail::get_layout (utils.hpp:238-246)."""
        return layout(lib.pfft_desc_layout(C.byref(self._c()), int(dir)))

    def validate(self):
        """detail::validate::validate_descriptor (descriptor_validation.hpp:264-281); needs no device."""
        _check(lib.pfft_desc_validate(C.byref(self._c())))

    def commit(self, queue=None):
        """descriptor::commit(queue) (descriptor.hpp:152-156).  `queue` is a HIP stream: a torch.cuda.Stream, a raw
        hipStream_t value, or None for torch's current stream (the default stream without torch)."""
        return committed_descriptor(self, queue)


class real_descriptor(descriptor):
    """A real-to-complex / complex-to-real 1-D transform of even `length` (PFFT_EXT_REAL_TRANSFORMS: an extension, the
    reference refuses the REAL domain and so does a plain descriptor(..., domain.REAL)).  Forward domain: `length`
    real scalars per transform (forward_distance / forward_offset in scalars); backward domain: length / 2 + 1 complex
    bins (backward_distance / backward_offset in complex elements).  compute_forward is numpy's rfft, compute_backward
    length * irfft.  In place: placement = IN_PLACE with forward_distance = 2 * backward_distance (padded rows)."""

    extensions = _lib.EXT_REAL_TRANSFORMS

    def __init__(self, length, scalar="f32"):
        super().__init__([int(length)], scalar, domain.REAL)
        self.backward_distance = int(length) // 2 + 1

    def _c(self):
        d = super()._c()
        d.extensions = self.extensions
        return d


class any_length_descriptor(descriptor):
    """A complex descriptor that may also be committed for 1-D lengths with a prime factor above 61, which a plain
    descriptor refuses like the reference (PFFT_EXT_ANY_LENGTH: Bluestein's algorithm in one kernel; fp32 lengths up to
    4096, fp64 up to 2048, interleaved storage, unit strides, any distance / offset / scale / batch, in place or out of
    place).  The bit is a permission: every length a plain descriptor takes gets the same plan and the same bits."""

    extensions = _lib.EXT_ANY_LENGTH

    def __init__(self, lengths, scalar="f32"):
        super().__init__(lengths, scalar, domain.COMPLEX)

    def _c(self):
        d = super()._c()
        d.extensions = self.extensions
        return d


class convolution_descriptor(descriptor):
    """A complex 1-D descriptor whose committed form also convolves (PFFT_EXT_CONVOLUTION: forward transform, product
    with a filter spectrum and backward transform in one kernel; fp32 / fp64, interleaved storage, unit strides, any
    distance >= length / offset / scale / batch, in place or out of place, lengths with a one-kernel LDS-resident plan).
    The bit is a permission plus the verbs set_filter / convolve / correlate: compute_forward and compute_backward are
    the plain descriptor's, same plan and same bits, so the filter spectrum can be made with the same plan."""

    extensions = _lib.EXT_CONVOLUTION

    def __init__(self, lengths, scalar="f32"):
        super().__init__(lengths, scalar, domain.COMPLEX)

    def _c(self):
        d = super()._c()
        d.extensions = self.extensions
        return d


class real_convolution_descriptor(real_descriptor):
    """A real 1-D descriptor whose committed form also convolves and filters REAL data (PFFT_EXT_REAL_CONVOLUTION: the
    R2C half, the product with a filter's half spectrum and the C2R half in one kernel that runs length / 2-point passes
    and moves every sample as one scalar).  A real_descriptor in every other respect -- the same rules, counts, distances,
    offsets and padded in-place pair -- and compute_forward / compute_backward are the real_descriptor's, same kernels
    and same bits, so a filter spectrum can be made with the same plan.  The committed form's verbs: set_filter takes
    (F, length / 2 + 1) complex bins, convolve / correlate take and give rows of `length` real scalars laid out as the
    forward domain, set_filter_taps takes (F, K) real taps and filter real signals."""

    extensions = _lib.EXT_REAL_CONVOLUTION


def _stream_handle(queue):
    if queue is None:
        try:
            import torch
            if torch.cuda.is_available():
                return int(torch.cuda.current_stream().cuda_stream)
        except ImportError:
            pass
        return 0
    if hasattr(queue, "cuda_stream"):
        return int(queue.cuda_stream)
    return int(queue)


def _ptr(x):
    """device pointer of a torch tensor / object with data_ptr() / raw integer"""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    return int(x)


def _is_complex(x):
    f = getattr(x, "is_complex", None)
    return bool(f()) if callable(f) else False


class event:
    """sycl::event of the reference: the completion of ONE compute_* submission (a hipEvent_t recorded behind its last
    kernel).  wait() blocks the host; pass it in another call's `dependencies` to order that call behind it."""

    def __init__(self, handle=None, plan=None):
        self._h = handle
        self._plan = plan  # keeps the plan alive; wait() on an event-less submission falls back to the stream

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.pfft_event_destroy(h)

    @property
    def native(self):
        return self._h

    def wait(self):
        if self._h:
            _check(lib.pfft_event_wait(self._h))
        elif self._plan is not None:
            self._plan.wait()
        return self

    def is_complete(self):
        if not self._h:
            return True
        done = C.c_int32(1)
        _check(lib.pfft_event_query(self._h, C.byref(done)))
        return bool(done.value)


def _dep_handle(d):
    """hipEvent_t of a dependency: an `event`, a torch.cuda.Event or a raw handle"""
    if isinstance(d, event):
        return d.native
    if hasattr(d, "cuda_event"):
        return int(d.cuda_event)
    return int(d) if d else None


class committed_descriptor:
    """portfft::committed_descriptor<Scalar, Domain> (committed_descriptor.hpp:46-315)."""

    def __init__(self, desc, queue=None, _clone_of=None):
        self._plan = C.c_void_p()
        if _clone_of is not None:
            # a copy shares the parent's snapshot: nothing is re-derived from a descriptor the user may have changed
            _check(lib.pfft_plan_clone(_clone_of._plan, C.byref(self._plan)))
            for name in ("params", "_device", "_torch", "_split", "_counts", "_scalar", "_real_dtype", "_cplx_dtype",
                         "_real", "_conv", "_rconv", "_pairs_prepared"):
                if hasattr(_clone_of, name):
                    setattr(self, name, getattr(_clone_of, name))
            self._no_deps = (C.c_void_p * 1)()
            return
        # the committed descriptor is a snapshot (the reference copies `params` at commit): the user's descriptor can be
        # modified and committed again without touching this plan
        self.params = _copy.deepcopy(desc)
        desc = self.params
        c = desc._c()
        _check(lib.pfft_plan_create(C.byref(c), C.c_void_p(_stream_handle(queue)), C.byref(self._plan)))
        self._device = None
        self._torch = None
        try:
            import torch
            self._torch = torch
            if torch.cuda.is_available():
                # the plan lives on the device of its queue: a torch stream knows its device, anything else was
                # committed on the current one
                dev = getattr(queue, "device", None)
                self._device = dev.index if dev is not None and getattr(dev, "index", None) is not None \
                    else torch.cuda.current_device()
        except ImportError:
            pass
        # element counts, storage and the dtypes a buffer may have are fixed here, so that a compute call costs a few
        # attribute reads
        self._split = desc.complex_storage == complex_storage.SPLIT_COMPLEX
        self._counts = {int(d): (desc.get_input_count(d), desc.get_output_count(d))
                        for d in (direction.FORWARD, direction.BACKWARD)}
        self._scalar = desc.scalar
        self._real = isinstance(desc, real_descriptor)
        self._rconv = isinstance(desc, real_convolution_descriptor)  # (then also _real: compute_* are the real plan's)
        self._conv = self._rconv or isinstance(desc, convolution_descriptor)
        if self._torch is not None:
            t = self._torch
            self._real_dtype, self._cplx_dtype = {"f64": (t.float64, t.complex128), "f16": (t.float16, t.complex32)}.get(
                desc.scalar, (t.float32, t.complex64))
        self._no_deps = (C.c_void_p * 1)()

    def __del__(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan:
            lib.pfft_plan_destroy(plan)

    def copy(self):
        """the reference's copy constructor (committed_descriptor_impl.hpp:774-817): shares kernels and twiddles,
        owns its scratch"""
        return committed_descriptor(self.params, _clone_of=self)

    __copy__ = copy

    def info(self):
        out = _lib.pfft_plan_info_t()
        _check(lib.pfft_plan_get_info(self._plan, C.byref(out)))
        return out

    def _check_real_buffer(self, x, count, complex_side, what):
        """a buffer of a real plan: `count` scalars on the real side, `count` complex elements on the complex side (a
        real-typed tensor there counts two scalars per element)"""
        if self._torch is None or not isinstance(x, self._torch.Tensor):
            return
        if complex_side:
            return self._check_buffer(x, count, False, what)
        if x.dtype == self._cplx_dtype:  # a complex view of the real rows (in place)
            return self._check_buffer(x, (count + 1) // 2, False, what)
        self._check_buffer(x, count, True, what)

    def _compute_real(self, dir, args, dep_arr, n_deps, ev_ref):
        n_in, n_out = self._counts[int(dir)]
        fwd = int(dir) == int(direction.FORWARD)
        if len(args) == 1:  # in place: one buffer that holds both domains (padded rows)
            self._check_real_buffer(args[0], n_in, not fwd, "inout")
            self._check_real_buffer(args[0], n_out, fwd, "inout")
            args = (args[0], args[0])
        elif len(args) == 2:
            self._check_real_buffer(args[0], n_in, not fwd, "in")
            self._check_real_buffer(args[1], n_out, fwd, "out")
        else:
            raise invalid_configuration("compute_* of a real plan takes (inout) or (in, out)")
        _check(lib.pfft_execute_ex(self._plan, int(dir), _ptr(args[0]), _ptr(args[1]), n_deps, dep_arr, ev_ref))

    def _check_buffer(self, x, count, split_plane, what):
        """a torch tensor handed to compute_* must live on the plan's device, have the descriptor's element type, be
        contiguous and cover the descriptor's element count (raw pointers cannot be checked)"""
        if self._torch is None or not isinstance(x, self._torch.Tensor):
            return
        if not x.is_cuda:
            raise invalid_configuration("%s: the buffer is not in device memory" % what)
        if self._device is not None and x.device.index != self._device:
            raise invalid_configuration("%s: the buffer lives on device %s, the plan was committed on device %d"
                                        % (what, x.device.index, self._device))
        dt = x.dtype
        if split_plane:
            unit = 1
            ok = dt == self._real_dtype
        else:
            ok = dt == self._cplx_dtype or dt == self._real_dtype  # a real view counts two scalars per element
            unit = 2 if dt == self._real_dtype else 1
        if not ok:
            raise invalid_configuration("%s: dtype %s does not match the descriptor (%s %s storage)"
                                        % (what, dt, self._scalar, "split" if split_plane else "interleaved"))
        if not x.is_contiguous():
            raise invalid_configuration("%s: the buffer must be contiguous" % what)
        if x.numel() < count * unit:
            raise invalid_configuration("%s: %d elements, the descriptor addresses %d" % (what, x.numel() // unit, count))

    def _marshal(self, dependencies, want_event):
        """what the _ex entry points take: the dependencies' handles as an array and their number, the slot of the
        completion event and its reference (None: no event is recorded)"""
        if dependencies:
            deps = [h for h in (_dep_handle(d) for d in dependencies) if h]
            dep_arr = (C.c_void_p * max(len(deps), 1))(*deps)
            n_deps = len(deps)
        else:
            dep_arr, n_deps = self._no_deps, 0
        ev = C.c_void_p()
        return dep_arr, n_deps, ev, C.byref(ev) if want_event else None

    def _require_on_device(self, verb, tensors):
        """the (name, tensor) pairs of `verb` live in device memory, on the plan's device"""
        for name, a in tensors:
            if not a.is_cuda:
                raise invalid_configuration("%s: the %s tensor is not in device memory" % (verb, name))
            if self._device is not None and a.device.index != self._device:
                raise invalid_configuration("%s: the %s tensor lives on device %s, the plan was committed on device %d"
                                            % (verb, name, a.device.index, self._device))

    def _require_real(self, verb):
        if not getattr(self, "_real", False):
            raise invalid_configuration("%s: the descriptor is not of the REAL domain (real_descriptor, "
                                        "real_convolution_descriptor)" % verb)

    def _set_window(self, verb, setter, w, frames=1):
        """set_window / set_synthesis_window / set_mdct_window / set_imdct_window / set_periodogram_window: None, or a device tensor of shape (frames * N,) of the
        real type"""
        self._require_real(verb)
        n = frames * int(self.params.lengths[0])
        if w is None:
            _check(setter(self._plan, None))
            return
        if self._torch is None or not isinstance(w, self._torch.Tensor):
            raise invalid_configuration("%s takes a torch tensor of shape (N,) or None" % verb)
        if w.dim() != 1 or w.shape[0] != n:
            raise invalid_configuration("%s: a window of shape (%d,) is needed, got %s" % (verb, n, tuple(w.shape)))
        if w.dtype != self._real_dtype:
            raise invalid_configuration("%s: dtype %s does not match the descriptor (%s real scalars)"
                                        % (verb, w.dtype, self._scalar))
        self._check_buffer(w, n, True, "window")
        _check(setter(self._plan, _ptr(w)))

    def _compute(self, dir, args, dependencies=None, want_event=True):
        n = len(args)
        split = self._split
        n_in, n_out = self._counts[int(dir)]
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        if getattr(self, "_real", False):
            self._compute_real(dir, args, dep_arr, n_deps, ev_ref)
        elif n == 1:  # in-place interleaved (committed_descriptor.hpp:171-176, 215-218)
            self._check_buffer(args[0], max(n_in, n_out), False, "inout")
            _check(lib.pfft_execute_ex(self._plan, int(dir), _ptr(args[0]), _ptr(args[0]), n_deps, dep_arr, ev_ref))
        elif n == 2 and split and not _is_complex(args[0]):
            # in-place split (committed_descriptor.hpp:186-192, 228-232)
            for a, w in zip(args, ("inout_real", "inout_imag")):
                self._check_buffer(a, max(n_in, n_out), True, w)
            _check(lib.pfft_execute_split_ex(self._plan, int(dir), _ptr(args[0]), _ptr(args[1]), _ptr(args[0]),
                                             _ptr(args[1]), n_deps, dep_arr, ev_ref))
        elif n == 2:  # out-of-place interleaved (committed_descriptor.hpp:242-246, 288-293)
            self._check_buffer(args[0], n_in, False, "in")
            self._check_buffer(args[1], n_out, False, "out")
            _check(lib.pfft_execute_ex(self._plan, int(dir), _ptr(args[0]), _ptr(args[1]), n_deps, dep_arr, ev_ref))
        elif n == 4:  # out-of-place split (committed_descriptor.hpp:258-263, 305-310)
            for a, w, c in zip(args, ("in_real", "in_imag", "out_real", "out_imag"), (n_in, n_in, n_out, n_out)):
                self._check_buffer(a, c, True, w)
            _check(lib.pfft_execute_split_ex(self._plan, int(dir), _ptr(args[0]), _ptr(args[1]), _ptr(args[2]),
                                             _ptr(args[3]), n_deps, dep_arr, ev_ref))
        else:
            raise invalid_configuration("compute_* takes (inout), (in, out), (inout_re, inout_im) or "
                                        "(in_re, in_im, out_re, out_im)")
        return event(ev.value if want_event else None, self)

    def compute_forward(self, *args, dependencies=None, want_event=True):
        """the USM overloads of committed_descriptor.hpp:171-310; `dependencies`: events (this module's, torch.cuda.Event
        or raw hipEvent_t) that must complete first; returns the event of this submission (want_event=False skips
        recording one: the returned object's wait() then waits for the plan's whole stream)."""
        return self._compute(direction.FORWARD, args, dependencies, want_event)

    def compute_backward(self, *args, dependencies=None, want_event=True):
        return self._compute(direction.BACKWARD, args, dependencies, want_event)

    # -- fused convolution (convolution_descriptor; no reference equivalent) ---------------------------------------
    def set_filter(self, spectra):
        """The filter spectra of convolve / correlate: a tensor of shape (F, N) or (N,) of the descriptor's complex type,
        in the frequency domain (what compute_forward of this plan makes of a filter).  Copied on the plan's stream into
        memory the plan owns: later writes to `spectra` do not matter, executes already submitted keep their filter.  Row t
        of an execute uses filter t mod F.  A copy() shares the filter until either side sets another."""
        if not getattr(self, "_conv", False):
            raise invalid_configuration("set_filter: the descriptor is not a convolution_descriptor")
        n = int(self.params.lengths[0])
        if getattr(self, "_rconv", False):  # a real plan: the length / 2 + 1 bins of the half spectrum
            n = n // 2 + 1
        count = 1
        if self._torch is not None and isinstance(spectra, self._torch.Tensor):
            if spectra.dim() not in (1, 2) or spectra.shape[-1] != n or spectra.numel() == 0:
                raise invalid_configuration("set_filter: a filter of shape (F, %d) or (%d,) is needed, got %s"
                                            % (n, n, tuple(spectra.shape)))
            if spectra.dtype != self._cplx_dtype:
                raise invalid_configuration("set_filter: dtype %s does not match the descriptor (%s interleaved storage)"
                                            % (spectra.dtype, self._scalar))
            count = spectra.numel() // n
            self._check_buffer(spectra, count * n, False, "filter")
        else:
            raise invalid_configuration("set_filter takes a torch tensor of shape (F, N) or (N,)")
        _check(lib.pfft_plan_set_filter(self._plan, _ptr(spectra), count))

    def _convolve(self, mode, args, dependencies, want_event):
        if not getattr(self, "_conv", False):
            raise invalid_configuration("convolve / correlate: the descriptor is not a convolution_descriptor")
        n_in, n_out = self._counts[int(direction.FORWARD)]
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        if len(args) not in (1, 2):
            raise invalid_configuration("convolve / correlate take (inout) or (in, out)")
        if getattr(self, "_rconv", False):  # real rows on both sides, laid out as the forward domain
            for a, w in zip(args, ("inout",) if len(args) == 1 else ("in", "out")):
                self._check_real_buffer(a, n_in, False, w)
            args = (args[0], args[-1])
        elif len(args) == 1:
            self._check_buffer(args[0], max(n_in, n_out), False, "inout")
            args = (args[0], args[0])
        else:
            self._check_buffer(args[0], n_in, False, "in")
            self._check_buffer(args[1], n_out, False, "out")
        _check(lib.pfft_execute_convolve_ex(self._plan, mode, _ptr(args[0]), _ptr(args[1]), n_deps, dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    def convolve(self, *args, dependencies=None, want_event=True):
        """out[t] = forward_scale * backward_scale * N * ifft(fft(in[t]) * H[t mod F]) in NumPy's terms -- what
        compute_forward, a multiply and compute_backward produce -- in one kernel.  `in` is laid out as the forward
        domain, `out` as the backward domain; (inout) convolves in place.  Arguments as compute_forward."""
        return self._convolve(_lib.CONVOLVE, args, dependencies, want_event)

    def correlate(self, *args, dependencies=None, want_event=True):
        """convolve with conj(H): the adjoint, what a backward pass through a convolution needs"""
        return self._convolve(_lib.CORRELATE, args, dependencies, want_event)

    # -- overlap-save FIR filtering of long signals (convolution_descriptor; no reference equivalent) ----------------
    def set_filter_taps(self, taps):
        """The filters of filter(), as time-domain taps: a tensor of shape (F, K) or (K,) of the descriptor's complex
        type, 1 <= K <= N.  The plan zero-pads every filter to N and transforms it on the device, unscaled; the spectra
        become the plan's filter as with set_filter, so convolve / correlate on them give the circular convolution with
        the padded taps.  Signal i of filter() uses filter i mod F."""
        if not getattr(self, "_conv", False):
            raise invalid_configuration("set_filter_taps: the descriptor is not a convolution_descriptor")
        n = int(self.params.lengths[0])
        if self._torch is None or not isinstance(taps, self._torch.Tensor):
            raise invalid_configuration("set_filter_taps takes a torch tensor of shape (F, K) or (K,)")
        if taps.dim() not in (1, 2) or taps.numel() == 0 or not 1 <= taps.shape[-1] <= n:
            raise invalid_configuration("set_filter_taps: taps of shape (F, K) or (K,) with 1 <= K <= %d are needed, got %s"
                                        % (n, tuple(taps.shape)))
        rconv = getattr(self, "_rconv", False)  # a real plan takes real taps
        if taps.dtype != (self._real_dtype if rconv else self._cplx_dtype):
            raise invalid_configuration("set_filter_taps: dtype %s does not match the descriptor (%s %s)"
                                        % (taps.dtype, self._scalar, "real scalars" if rconv else "interleaved storage"))
        k = int(taps.shape[-1])
        count = taps.numel() // k
        self._check_buffer(taps, count * k, rconv, "taps")
        _check(lib.pfft_plan_set_filter_taps(self._plan, _ptr(taps), k, count))

    def filter(self, x, y, correlate=False, dependencies=None, want_event=True):
        """Linear convolution (correlate=True: correlation) of the signals `x` with the taps of set_filter_taps, into `y`,
        in one kernel launch (overlap-save in segments of N points).  `x`, `y`: device tensors of the descriptor's
        complex type, 1-D (one signal) or 2-D (signal, sample) with unit inner stride; the pitch of a signal is stride(0),
        the lengths are shape[-1], and both hold the same number of signals.  In NumPy's terms, with c = forward_scale *
        backward_scale * N and h the taps of filter i mod F:
          y[i] = c * np.convolve(x[i], h)[:y.shape[-1]]                               (y.shape[-1] <= x.shape[-1] + K - 1)
          y[i] = c * np.correlate(concatenate(x[i], zeros(K - 1)), h, "valid")[:y.shape[-1]]   (y.shape[-1] <= x.shape[-1])
        Only y[i, :] is written.  x and y must not overlap.  With real taps the real and the imaginary part of a signal
        are filtered independently."""
        if not getattr(self, "_conv", False):
            raise invalid_configuration("filter: the descriptor is not a convolution_descriptor")
        t = self._torch
        rconv = getattr(self, "_rconv", False)  # a real plan filters real signals; lengths and pitches count scalars
        sample_dtype = self._real_dtype if rconv else self._cplx_dtype
        for name, a in (("in", x), ("out", y)):
            if t is None or not isinstance(a, t.Tensor):
                raise invalid_configuration("filter takes torch tensors (in, out)")
            if a.dim() not in (1, 2) or a.numel() == 0:
                raise invalid_configuration("filter: the %s tensor must be 1-D or 2-D (signal, sample) and not empty, got "
                                            "shape %s" % (name, tuple(a.shape)))
            if a.dtype != sample_dtype:
                raise invalid_configuration("filter: dtype %s of the %s tensor does not match the descriptor (%s %s)"
                                            % (a.dtype, name, self._scalar, "real scalars" if rconv else "interleaved storage"))
            if a.stride(-1) != 1 and a.shape[-1] > 1:
                raise invalid_configuration("filter: the %s tensor needs unit inner stride, got %d" % (name, a.stride(-1)))
            if a.dim() == 2 and a.shape[0] > 1 and a.stride(0) < a.shape[1]:
                raise invalid_configuration("filter: the signals of the %s tensor overlap (stride %d below the length %d)"
                                            % (name, a.stride(0), a.shape[1]))
        n_x = int(x.shape[0]) if x.dim() == 2 else 1
        n_y = int(y.shape[0]) if y.dim() == 2 else 1
        if n_x != n_y:
            raise invalid_configuration("filter: %d input signals but %d output signals" % (n_x, n_y))
        self._require_on_device("filter", (("in", x), ("out", y)))
        in_len, out_len = int(x.shape[-1]), int(y.shape[-1])
        in_pitch = int(x.stride(0)) if x.dim() == 2 and n_x > 1 else in_len
        out_pitch = int(y.stride(0)) if y.dim() == 2 and n_y > 1 else out_len
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_filter_ex(self._plan, _lib.CORRELATE if correlate else _lib.CONVOLVE, _ptr(x), _ptr(y), n_x,
                                          in_len, in_pitch, out_len, out_pitch, n_deps, dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    # -- short-time Fourier transform of real signals (every plan of the REAL domain; no reference equivalent) -------
    def set_window(self, w):
        """The window of stft(): a device tensor of shape (N,) of the descriptor's real type, or None for all ones.  The
        first call resolves the kernel (a length without a pre-compiled one is compiled here); every call copies the
        window on the plan's stream into memory the plan owns, so later writes to `w` do not matter and executes already
        submitted keep their window.  A copy() shares the window until either side sets another."""
        self._set_window("set_window", lib.pfft_plan_set_window, w)

    def stft(self, x, y, hop, lead=0, pad="zero", dependencies=None, want_event=True):
        """Short-time Fourier transform of the real signals `x` with the window of set_window, into `y`, in one kernel
        launch.  `x`: (S, L) or (L,) of the descriptor's real type, unit inner stride, signal pitch stride(0).  `y`:
        (S, F, M + 1) or (F, M + 1) of its complex type, M = N / 2, unit inner stride; the pitches of a frame and of a
        signal are its strides, F = y.shape[-2] frames are computed.  In NumPy's terms, with xe the signal extended by
        zeros (pad="zero") or np.pad(mode="reflect") (pad="reflect"):
          y[i, f] = forward_scale * np.fft.rfft(w * xe[i, f * hop - lead : f * hop - lead + N])
        torch.stft(x, N, hop, window=w, center=True) is lead = N // 2, pad="reflect", F = 1 + L // hop, transposed.  Only
        y[i, f, :] is written; x and y must not overlap."""
        self._require_real("stft")
        t = self._torch
        n = int(self.params.lengths[0])
        m = n // 2
        if t is None or not isinstance(x, t.Tensor) or not isinstance(y, t.Tensor):
            raise invalid_configuration("stft takes torch tensors (in, out)")
        if pad not in ("zero", "reflect"):
            raise invalid_configuration("stft: pad must be \"zero\" or \"reflect\", got %r" % (pad,))
        if x.dim() not in (1, 2) or x.numel() == 0:
            raise invalid_configuration("stft: the in tensor must be 1-D or 2-D (signal, sample) and not empty, got shape %s"
                                        % (tuple(x.shape),))
        if y.dim() != x.dim() + 1 or y.numel() == 0:
            raise invalid_configuration("stft: the out tensor must be %d-D (%sframe, bin) and not empty, got shape %s"
                                        % (x.dim() + 1, "signal, " if x.dim() == 2 else "", tuple(y.shape)))
        if x.dtype != self._real_dtype:
            raise invalid_configuration("stft: dtype %s of the in tensor does not match the descriptor (%s real scalars)"
                                        % (x.dtype, self._scalar))
        if y.dtype != self._cplx_dtype:
            raise invalid_configuration("stft: dtype %s of the out tensor does not match the descriptor (%s interleaved "
                                        "storage)" % (y.dtype, self._scalar))
        if y.shape[-1] != m + 1:
            raise invalid_configuration("stft: the out tensor holds %d bins per frame, a frame of %d scalars has %d"
                                        % (y.shape[-1], n, m + 1))
        n_x = int(x.shape[0]) if x.dim() == 2 else 1
        n_y = int(y.shape[0]) if y.dim() == 3 else 1
        if n_x != n_y:
            raise invalid_configuration("stft: %d input signals but %d output signals" % (n_x, n_y))
        for name, a in (("in", x), ("out", y)):
            if a.stride(-1) != 1 and a.shape[-1] > 1:
                raise invalid_configuration("stft: the %s tensor needs unit inner stride, got %d" % (name, a.stride(-1)))
        in_len, n_frames = int(x.shape[-1]), int(y.shape[-2])
        in_pitch = int(x.stride(0)) if x.dim() == 2 and n_x > 1 else in_len
        frame_pitch = int(y.stride(-2)) if n_frames > 1 else m + 1
        out_pitch = int(y.stride(0)) if y.dim() == 3 and n_y > 1 else n_frames * frame_pitch
        if in_pitch < in_len:
            raise invalid_configuration("stft: the signals of the in tensor overlap (stride %d below the length %d)"
                                        % (in_pitch, in_len))
        if frame_pitch < m + 1:
            raise invalid_configuration("stft: the frames of the out tensor overlap (frame stride %d below the %d bins)"
                                        % (frame_pitch, m + 1))
        if out_pitch < n_frames * frame_pitch:
            raise invalid_configuration("stft: the signals of the out tensor overlap (stride %d below %d frames of pitch %d)"
                                        % (out_pitch, n_frames, frame_pitch))
        hop, lead = int(hop), int(lead)
        if hop < 1:
            raise invalid_configuration("stft: hop %d, must be at least 1" % hop)
        if not 0 <= lead < n:
            raise invalid_configuration("stft: lead %d, must be in [0, %d)" % (lead, n))
        last = (n_frames - 1) * hop
        if pad == "zero":
            if last >= in_len + lead:
                raise invalid_configuration("stft: frame %d starts at sample %d - lead %d, beyond the in_length %d: every "
                                            "frame must hold at least one sample (n_frames, hop)"
                                            % (n_frames - 1, last, lead, in_len))
        else:
            if lead > in_len - 1:
                raise invalid_configuration("stft: lead %d above in_length - 1 = %d: reflection mirrors an index at most once"
                                            % (lead, in_len - 1))
            if last + n > in_len + 2 * lead:
                raise invalid_configuration("stft: frame %d ends at sample %d - lead %d, beyond the signal of in_length %d "
                                            "reflected by lead on both sides (n_frames, hop)"
                                            % (n_frames - 1, last + n, lead, in_len))
        self._require_on_device("stft", (("in", x), ("out", y)))
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_stft_ex(self._plan, _ptr(x), _ptr(y), n_x, in_len, in_pitch, hop, lead,
                                        _lib.PAD_REFLECT if pad == "reflect" else _lib.PAD_ZERO, n_frames, frame_pitch,
                                        out_pitch, n_deps, dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    # -- inverse short-time Fourier transform, overlap-add synthesis (every plan of the REAL domain) -------------------
    def set_synthesis_window(self, w):
        """The window of istft(): a device tensor of shape (N,) of the descriptor's real type, or None for all ones;
        independent of set_window (pass the same tensor to both for torch's convention).  The first call resolves the
        kernel (a length without a pre-compiled one is compiled here); every call copies the window on the plan's stream
        into memory the plan owns.  A copy() shares the window until either side sets another."""
        self._set_window("set_synthesis_window", lib.pfft_plan_set_synthesis_window, w)

    def istft_chunk_frames(self, n_signals, n_frames, hop):
        """The chunk length istft(chunk_frames=0) chooses for that many signals and frames at that hop (a synthesis
        window must have been set): with H = ceil(N / hop) - 1 about H / chunk_frames of the frames are transformed twice."""
        out = C.c_uint64()
        _check(lib.pfft_plan_istft_chunk_frames(self._plan, int(n_signals), int(n_frames), int(hop), C.byref(out)))
        return int(out.value)

    def istft(self, y, x, hop, lead=0, normalize=False, chunk_frames=0, dependencies=None, want_event=True):
        """Inverse short-time Fourier transform (overlap-add) of the bins `y` with the window of set_synthesis_window,
        into the real signals `x`, in one kernel launch.  `y`: (S, F, M + 1) or (F, M + 1) of the descriptor's complex
        type, M = N / 2, as stft() writes it; `x`: (S, L) or (L,) of its real type; strides as in stft().  In NumPy's
        terms, with g[i, f] = backward_scale * N * np.fft.irfft(y[i, f], N) and u = t + lead:
          x[i, t] = sum over f of w[u - f * hop] * g[i, f, u - f * hop]        (the frames with 0 <= u - f * hop < N)
        and normalize=True divides by sum over f of w[u - f * hop] ** 2 (exactly 0 where that is not above 1e-11).
        torch.istft(Y, N, hop, window=w, center=True, length=L) is backward_scale = 1 / N, lead = N // 2,
        normalize=True, transposed.  The sums run in ascending f whatever chunk_frames is (0: the plan chooses), so the
        result does not depend on it.  Only x[i, :L] is written; x and y must not overlap."""
        self._require_real("istft")
        t = self._torch
        n = int(self.params.lengths[0])
        m = n // 2
        if t is None or not isinstance(x, t.Tensor) or not isinstance(y, t.Tensor):
            raise invalid_configuration("istft takes torch tensors (in, out)")
        if x.dim() not in (1, 2) or x.numel() == 0:
            raise invalid_configuration("istft: the out tensor must be 1-D or 2-D (signal, sample) and not empty, got shape %s"
                                        % (tuple(x.shape),))
        if y.dim() != x.dim() + 1 or y.numel() == 0:
            raise invalid_configuration("istft: the in tensor must be %d-D (%sframe, bin) and not empty, got shape %s"
                                        % (x.dim() + 1, "signal, " if x.dim() == 2 else "", tuple(y.shape)))
        if y.dtype != self._cplx_dtype:
            raise invalid_configuration("istft: dtype %s of the in tensor does not match the descriptor (%s interleaved "
                                        "storage)" % (y.dtype, self._scalar))
        if x.dtype != self._real_dtype:
            raise invalid_configuration("istft: dtype %s of the out tensor does not match the descriptor (%s real scalars)"
                                        % (x.dtype, self._scalar))
        if y.shape[-1] != m + 1:
            raise invalid_configuration("istft: the in tensor holds %d bins per frame, a frame of %d scalars has %d"
                                        % (y.shape[-1], n, m + 1))
        n_x = int(x.shape[0]) if x.dim() == 2 else 1
        n_y = int(y.shape[0]) if y.dim() == 3 else 1
        if n_x != n_y:
            raise invalid_configuration("istft: %d input signals but %d output signals" % (n_y, n_x))
        for name, a in (("in", y), ("out", x)):
            if a.stride(-1) != 1 and a.shape[-1] > 1:
                raise invalid_configuration("istft: the %s tensor needs unit inner stride, got %d" % (name, a.stride(-1)))
        out_len, n_frames = int(x.shape[-1]), int(y.shape[-2])
        out_pitch = int(x.stride(0)) if x.dim() == 2 and n_x > 1 else out_len
        frame_pitch = int(y.stride(-2)) if n_frames > 1 else m + 1
        in_pitch = int(y.stride(0)) if y.dim() == 3 and n_y > 1 else n_frames * frame_pitch
        if out_pitch < out_len:
            raise invalid_configuration("istft: the signals of the out tensor overlap (stride %d below the length %d)"
                                        % (out_pitch, out_len))
        if frame_pitch < m + 1:
            raise invalid_configuration("istft: the frames of the in tensor overlap (frame stride %d below the %d bins)"
                                        % (frame_pitch, m + 1))
        if in_pitch < n_frames * frame_pitch:
            raise invalid_configuration("istft: the signals of the in tensor overlap (stride %d below %d frames of pitch %d)"
                                        % (in_pitch, n_frames, frame_pitch))
        hop, lead, chunk_frames = int(hop), int(lead), int(chunk_frames)
        if hop < 1:
            raise invalid_configuration("istft: hop %d, must be at least 1" % hop)
        if hop > n:
            raise invalid_configuration("istft: hop %d above the frame length %d leaves gaps that no frame covers" % (hop, n))
        if not 0 <= lead < n:
            raise invalid_configuration("istft: lead %d, must be in [0, %d)" % (lead, n))
        if chunk_frames < 0:
            raise invalid_configuration("istft: chunk_frames %d, must be at least 0 (0: the plan chooses)" % chunk_frames)
        last = (n_frames - 1) * hop
        if out_len + lead > last + n:
            raise invalid_configuration("istft: out_length %d above (n_frames - 1) * hop + N - lead = %d: the samples behind "
                                        "it are covered by no frame" % (out_len, last + n - lead))
        if last >= out_len + lead:
            raise invalid_configuration("istft: frame %d starts at sample %d - lead %d, beyond the out_length %d: every "
                                        "frame must contribute at least one sample (n_frames, hop)"
                                        % (n_frames - 1, last, lead, out_len))
        self._require_on_device("istft", (("in", y), ("out", x)))
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_istft_ex(self._plan, _ptr(y), _ptr(x), n_x, n_frames, frame_pitch, in_pitch, hop, lead,
                                         _lib.ISTFT_NORMALIZE if normalize else _lib.ISTFT_PLAIN, out_len, out_pitch,
                                         chunk_frames, n_deps, dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    # -- discrete cosine transforms of type 2 and 3 (every plan of the REAL domain; no reference equivalent) -----------
    def prepare_dct(self):
        """Make dct() available: resolves the two kernels (a length without pre-compiled ones is compiled here) and uploads
        their table of N / 2 + 1 twiddles into memory the plan owns.  Takes no data; a second call does nothing.  A copy()
        shares both.  dct() never prepares on its own."""
        self._require_real("prepare_dct")
        _check(lib.pfft_plan_prepare_dct(self._plan))

    def dct(self, x, y, type=2, dependencies=None, want_event=True):
        """Discrete cosine transform of the rows of `x` into `y` in one kernel launch: scipy.fft.dct(x, type, norm=None)
        times forward_scale (type=2) or backward_scale (type=3).  With the default scales type 3 of type 2 of x is
        2 * N * x.  `x`, `y`: (rows, N) or (N,) of the descriptor's real type, unit inner stride, row pitch stride(0), rows
        that do not overlap.  `y is x` transforms in place; otherwise x and y must not overlap.  Only y[r, :] is written."""
        self._require_real("dct")
        t = self._torch
        n = int(self.params.lengths[0])
        if t is None or not isinstance(x, t.Tensor) or not isinstance(y, t.Tensor):
            raise invalid_configuration("dct takes torch tensors (in, out)")
        if type not in (_lib.DCT_II, _lib.DCT_III):
            raise invalid_configuration("dct: type %r, must be 2 or 3" % (type,))
        for name, a in (("in", x), ("out", y)):
            if a.dim() not in (1, 2) or a.numel() == 0:
                raise invalid_configuration("dct: the %s tensor must be 1-D or 2-D (row, sample) and not empty, got shape %s"
                                            % (name, tuple(a.shape)))
            if a.dtype != self._real_dtype:
                raise invalid_configuration("dct: dtype %s of the %s tensor does not match the descriptor (%s real scalars)"
                                            % (a.dtype, name, self._scalar))
            if a.shape[-1] != n:
                raise invalid_configuration("dct: the last dimension of the %s tensor is %d, the descriptor's length is %d"
                                            % (name, a.shape[-1], n))
            if a.stride(-1) != 1:
                raise invalid_configuration("dct: the %s tensor needs unit inner stride, got %d" % (name, a.stride(-1)))
        n_x = int(x.shape[0]) if x.dim() == 2 else 1
        n_y = int(y.shape[0]) if y.dim() == 2 else 1
        if n_x != n_y:
            raise invalid_configuration("dct: %d input rows but %d output rows" % (n_x, n_y))
        in_pitch = int(x.stride(0)) if x.dim() == 2 and n_x > 1 else n
        out_pitch = int(y.stride(0)) if y.dim() == 2 and n_y > 1 else n
        for name, pitch in (("in", in_pitch), ("out", out_pitch)):
            if pitch < n:
                raise invalid_configuration("dct: the rows of the %s tensor overlap (stride %d below the length %d)"
                                            % (name, pitch, n))
        self._require_on_device("dct", (("in", x), ("out", y)))
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_dct_ex(self._plan, int(type), _ptr(x), _ptr(y), n_x, in_pitch, out_pitch, n_deps, dep_arr,
                                       ev_ref))
        return event(ev.value if want_event else None, self)

    # -- DCT-IV of real rows and MDCT of real signals (every plan of the REAL domain; no reference equivalent) ----------
    def prepare_dct4(self):
        """Make dct4() available: resolves the kernels (a length without pre-compiled ones is compiled here) and uploads
        their table of N twiddles into memory the plan owns.  Takes no data; a second call does nothing.  A copy() shares
        both.  dct4() never prepares on its own."""
        self._require_real("prepare_dct4")
        _check(lib.pfft_plan_prepare_dct4(self._plan))

    def dct4(self, x, y, inverse=False, dependencies=None, want_event=True):
        """Discrete cosine transform of type 4 of the rows of `x` into `y` in one kernel launch: scipy.fft.dct(x, 4,
        norm=None) times forward_scale, or times backward_scale with inverse=True.  The transform is its own inverse up to
        2N: with the default scales dct4 of dct4 of x is 2 * N * x.  `x`, `y`: (rows, N) or (N,) of the descriptor's real
        type, unit inner stride, row pitch stride(0), rows that do not overlap.  `y is x` transforms in place; otherwise x
        and y must not overlap.  Only y[r, :] is written."""
        self._require_real("dct4")
        t = self._torch
        n = int(self.params.lengths[0])
        if t is None or not isinstance(x, t.Tensor) or not isinstance(y, t.Tensor):
            raise invalid_configuration("dct4 takes torch tensors (in, out)")
        for name, a in (("in", x), ("out", y)):
            if a.dim() not in (1, 2) or a.numel() == 0:
                raise invalid_configuration("dct4: the %s tensor must be 1-D or 2-D (row, sample) and not empty, got shape %s"
                                            % (name, tuple(a.shape)))
            if a.dtype != self._real_dtype:
                raise invalid_configuration("dct4: dtype %s of the %s tensor does not match the descriptor (%s real scalars)"
                                            % (a.dtype, name, self._scalar))
            if a.shape[-1] != n:
                raise invalid_configuration("dct4: the last dimension of the %s tensor is %d, the descriptor's length is %d"
                                            % (name, a.shape[-1], n))
            if a.stride(-1) != 1:
                raise invalid_configuration("dct4: the %s tensor needs unit inner stride, got %d" % (name, a.stride(-1)))
        n_x = int(x.shape[0]) if x.dim() == 2 else 1
        n_y = int(y.shape[0]) if y.dim() == 2 else 1
        if n_x != n_y:
            raise invalid_configuration("dct4: %d input rows but %d output rows" % (n_x, n_y))
        in_pitch = int(x.stride(0)) if x.dim() == 2 and n_x > 1 else n
        out_pitch = int(y.stride(0)) if y.dim() == 2 and n_y > 1 else n
        for name, pitch in (("in", in_pitch), ("out", out_pitch)):
            if pitch < n:
                raise invalid_configuration("dct4: the rows of the %s tensor overlap (stride %d below the length %d)"
                                            % (name, pitch, n))
        self._require_on_device("dct4", (("in", x), ("out", y)))
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_dct4_ex(self._plan, 1 if inverse else 0, _ptr(x), _ptr(y), n_x, in_pitch, out_pitch, n_deps,
                                        dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    def set_mdct_window(self, w):
        """The window of mdct(): a device tensor of shape (2 * N,) of the descriptor's real type, or None for all ones.
        Does what prepare_dct4() does, then copies the window on the plan's stream into memory the plan owns; every call
        copies again.  A copy() shares the window until either side sets another."""
        self._set_window("set_mdct_window", lib.pfft_plan_set_mdct_window, w, frames=2)

    def mdct(self, x, y, lead=None, dependencies=None, want_event=True):
        """Modified discrete cosine transform of the real signals `x` with the window of set_mdct_window, into `y`, in one
        kernel launch.  `x`: (S, L) or (L,) of the descriptor's real type, unit inner stride, signal pitch stride(0).  `y`:
        (S, F, N) or (F, N) of the same type, unit inner stride; the pitches of a frame and of a signal are its strides,
        F = y.shape[-2] frames are computed.  A frame covers 2N samples and the hop is N.  With xe the signal extended by
        zeros and v = w * xe[i, f * N - lead : f * N - lead + 2 * N]:
          y[i, f, k] = forward_scale * 2 * sum_n v[n] cos(pi (2n + 1 + N)(2k + 1) / (4N))
        lead=None means N, the usual choice; any lead in [0, 2N) is taken.  Only y[i, f, :] is written; x and y must not
        overlap.  The inverse is imdct(): the unfold of dct4() of a coefficient row [p, q] to [q, -reverse(q), -reverse(p),
        -p], the window and the overlap-add at hop N give 2N * x for a Princen-Bradley window, lead = N and ceil(L / N) + 1
        frames."""
        self._require_real("mdct")
        t = self._torch
        n = int(self.params.lengths[0])
        if t is None or not isinstance(x, t.Tensor) or not isinstance(y, t.Tensor):
            raise invalid_configuration("mdct takes torch tensors (in, out)")
        if x.dim() not in (1, 2) or x.numel() == 0:
            raise invalid_configuration("mdct: the in tensor must be 1-D or 2-D (signal, sample) and not empty, got shape %s"
                                        % (tuple(x.shape),))
        if y.dim() != x.dim() + 1 or y.numel() == 0:
            raise invalid_configuration("mdct: the out tensor must be %d-D (%sframe, coefficient) and not empty, got shape %s"
                                        % (x.dim() + 1, "signal, " if x.dim() == 2 else "", tuple(y.shape)))
        for name, a in (("in", x), ("out", y)):
            if a.dtype != self._real_dtype:
                raise invalid_configuration("mdct: dtype %s of the %s tensor does not match the descriptor (%s real scalars)"
                                            % (a.dtype, name, self._scalar))
        if y.shape[-1] != n:
            raise invalid_configuration("mdct: the last dimension of the out tensor is %d, a frame has %d coefficients"
                                        % (y.shape[-1], n))
        n_x = int(x.shape[0]) if x.dim() == 2 else 1
        n_y = int(y.shape[0]) if y.dim() == 3 else 1
        if n_x != n_y:
            raise invalid_configuration("mdct: %d input signals but %d output signals" % (n_x, n_y))
        for name, a in (("in", x), ("out", y)):
            if a.stride(-1) != 1 and a.shape[-1] > 1:
                raise invalid_configuration("mdct: the %s tensor needs unit inner stride, got %d" % (name, a.stride(-1)))
        in_len, n_frames = int(x.shape[-1]), int(y.shape[-2])
        in_pitch = int(x.stride(0)) if x.dim() == 2 and n_x > 1 else in_len
        frame_pitch = int(y.stride(-2)) if n_frames > 1 else n
        out_pitch = int(y.stride(0)) if y.dim() == 3 and n_y > 1 else n_frames * frame_pitch
        if in_pitch < in_len:
            raise invalid_configuration("mdct: the signals of the in tensor overlap (stride %d below the length %d)"
                                        % (in_pitch, in_len))
        if frame_pitch < n:
            raise invalid_configuration("mdct: the frames of the out tensor overlap (frame stride %d below the %d "
                                        "coefficients)" % (frame_pitch, n))
        if out_pitch < n_frames * frame_pitch:
            raise invalid_configuration("mdct: the signals of the out tensor overlap (stride %d below %d frames of pitch %d)"
                                        % (out_pitch, n_frames, frame_pitch))
        lead = n if lead is None else int(lead)
        if not 0 <= lead < 2 * n:
            raise invalid_configuration("mdct: lead %d, must be in [0, %d)" % (lead, 2 * n))
        last = (n_frames - 1) * n
        if last >= in_len + lead:
            raise invalid_configuration("mdct: frame %d starts at sample %d - lead %d, beyond the in_length %d: every "
                                        "frame must hold at least one sample (n_frames; the hop is %d)"
                                        % (n_frames - 1, last, lead, in_len, n))
        self._require_on_device("mdct", (("in", x), ("out", y)))
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_mdct_ex(self._plan, _ptr(x), _ptr(y), n_x, in_len, in_pitch, lead, n_frames, frame_pitch,
                                        out_pitch, n_deps, dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    # -- inverse MDCT, windowed overlap-add synthesis (every plan of the REAL domain; no reference equivalent) ----------
    def set_imdct_window(self, w):
        """The synthesis window of imdct(): a device tensor of shape (2 * N,) of the descriptor's real type, or None for all
        ones; independent of set_mdct_window.  Does what prepare_dct4() does; the first call also resolves the kernel (a
        length without a pre-compiled one is compiled here); every call copies the window on the plan's stream into memory
        the plan owns.  A copy() shares the window until either side sets another."""
        self._set_window("set_imdct_window", lib.pfft_plan_set_imdct_window, w, frames=2)

    def imdct_chunk_frames(self, n_signals, n_frames):
        """The chunk length imdct(chunk_frames=0) chooses for that many signals and frames (a window must have been set):
        about 1 / chunk_frames of the frames are transformed twice."""
        self._require_real("imdct_chunk_frames")
        out = C.c_uint64()
        _check(lib.pfft_plan_imdct_chunk_frames(self._plan, int(n_signals), int(n_frames), C.byref(out)))
        return int(out.value)

    def imdct(self, y, x, lead=None, chunk_frames=0, dependencies=None, want_event=True):
        """Inverse modified discrete cosine transform of the coefficient frames `y` with the window of set_imdct_window,
        into the real signals `x`, in one kernel launch.  `y`: (S, F, N) or (F, N) of the descriptor's real type, as mdct()
        writes it; `x`: (S, L) or (L,) of the same type; strides as in mdct().  With [p, q] = the unscaled dct4 of y[i, f],
        g[i, f] = [q, -reverse(q), -reverse(p), -p] (2N scalars) and u = t + lead:
          x[i, t] = backward_scale * sum over f of w[u - f * N] * g[i, f, u - f * N]      (the frames with 0 <= u - f * N < 2N)
        lead=None means N, the usual choice; any lead in [0, 2N) is taken.  With the sine window in set_mdct_window and here,
        lead = N, F = ceil(L / N) + 1 and backward_scale = 1 / (2N), imdct(mdct(x)) is x.  The two frames of a sample are
        added in ascending f whatever chunk_frames is (0: the plan chooses), so the result does not depend on it.  Only
        x[i, :L] is written; x and y must not overlap."""
        self._require_real("imdct")
        t = self._torch
        n = int(self.params.lengths[0])
        if t is None or not isinstance(x, t.Tensor) or not isinstance(y, t.Tensor):
            raise invalid_configuration("imdct takes torch tensors (in, out)")
        if x.dim() not in (1, 2) or x.numel() == 0:
            raise invalid_configuration("imdct: the out tensor must be 1-D or 2-D (signal, sample) and not empty, got shape %s"
                                        % (tuple(x.shape),))
        if y.dim() != x.dim() + 1 or y.numel() == 0:
            raise invalid_configuration("imdct: the in tensor must be %d-D (%sframe, coefficient) and not empty, got shape %s"
                                        % (x.dim() + 1, "signal, " if x.dim() == 2 else "", tuple(y.shape)))
        for name, a in (("in", y), ("out", x)):
            if a.dtype != self._real_dtype:
                raise invalid_configuration("imdct: dtype %s of the %s tensor does not match the descriptor (%s real scalars)"
                                            % (a.dtype, name, self._scalar))
        if y.shape[-1] != n:
            raise invalid_configuration("imdct: the last dimension of the in tensor is %d, a frame has %d coefficients"
                                        % (y.shape[-1], n))
        n_x = int(x.shape[0]) if x.dim() == 2 else 1
        n_y = int(y.shape[0]) if y.dim() == 3 else 1
        if n_x != n_y:
            raise invalid_configuration("imdct: %d input signals but %d output signals" % (n_y, n_x))
        for name, a in (("in", y), ("out", x)):
            if a.stride(-1) != 1 and a.shape[-1] > 1:
                raise invalid_configuration("imdct: the %s tensor needs unit inner stride, got %d" % (name, a.stride(-1)))
        out_len, n_frames = int(x.shape[-1]), int(y.shape[-2])
        out_pitch = int(x.stride(0)) if x.dim() == 2 and n_x > 1 else out_len
        frame_pitch = int(y.stride(-2)) if n_frames > 1 else n
        in_pitch = int(y.stride(0)) if y.dim() == 3 and n_y > 1 else n_frames * frame_pitch
        if out_pitch < out_len:
            raise invalid_configuration("imdct: the signals of the out tensor overlap (stride %d below the length %d)"
                                        % (out_pitch, out_len))
        if frame_pitch < n:
            raise invalid_configuration("imdct: the frames of the in tensor overlap (frame stride %d below the %d "
                                        "coefficients)" % (frame_pitch, n))
        if in_pitch < n_frames * frame_pitch:
            raise invalid_configuration("imdct: the signals of the in tensor overlap (stride %d below %d frames of pitch %d)"
                                        % (in_pitch, n_frames, frame_pitch))
        lead = n if lead is None else int(lead)
        chunk_frames = int(chunk_frames)
        if not 0 <= lead < 2 * n:
            raise invalid_configuration("imdct: lead %d, must be in [0, %d)" % (lead, 2 * n))
        if chunk_frames < 0:
            raise invalid_configuration("imdct: chunk_frames %d, must be at least 0 (0: the plan chooses)" % chunk_frames)
        last = (n_frames - 1) * n
        if out_len + lead > last + 2 * n:
            raise invalid_configuration("imdct: out_length %d above (n_frames - 1) * N + 2N - lead = %d: the samples behind "
                                        "it are covered by no frame" % (out_len, last + 2 * n - lead))
        if last >= out_len + lead:
            raise invalid_configuration("imdct: frame %d starts at sample %d - lead %d, beyond the out_length %d: every "
                                        "frame must contribute at least one sample (n_frames; the hop is %d)"
                                        % (n_frames - 1, last, lead, out_len, n))
        self._require_on_device("imdct", (("in", y), ("out", x)))
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_imdct_ex(self._plan, _ptr(y), _ptr(x), n_x, n_frames, frame_pitch, in_pitch, lead, out_len,
                                         out_pitch, chunk_frames, n_deps, dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    # -- power spectrogram / Welch periodogram of real signals (every plan of the REAL domain; no reference equivalent) --
    def set_periodogram_window(self, w):
        """The window of periodogram(): a device tensor of shape (N,) of the descriptor's real type, or None for all ones;
        independent of set_window.  The first call resolves the kernel (a length without a pre-compiled one is compiled
        here); every call copies the window on the plan's stream into memory the plan owns.  A copy() shares the window
        until either side sets another."""
        self._set_window("set_periodogram_window", lib.pfft_plan_set_periodogram_window, w)

    def periodogram(self, x, p, hop, n_frames, frames_per_row=1, lead=0, pad="zero", dependencies=None, want_event=True):
        """Sums of squared short-time Fourier bins of the real signals `x` with the window of set_periodogram_window, into
        `p`, in one kernel launch: the complex bins never reach memory.  `x`: (S, L) or (L,) of the descriptor's real type,
        as in stft().  `p`: (S, R, M + 1) or (R, M + 1) of the SAME real type, M = N / 2, R = ceil(n_frames /
        frames_per_row), unit inner stride; the pitches of a row and of a signal are its strides.  With X[i, f] the frame
        stft() computes (forward_scale, window, hop, lead and pad as there):
          p[i, c] = sum over f in [c * frames_per_row, min((c + 1) * frames_per_row, n_frames)) of abs(X[i, f]) ** 2
        frames_per_row=1 is the power spectrogram, frames_per_row=n_frames Welch's sum (one row per signal).  A sum, not a
        mean, and without one-sided doubling: normalise afterwards, or through forward_scale (which enters squared).  The
        frames of a row are added in ascending f by one accumulator: the result does not depend on how many signals share
        a call, bit for bit.  One row is one unit of work: for a Welch estimate of a single long signal choose
        frames_per_row so that S * R is a few thousand and add the R rows with torch.  Only p[i, c, :] is written; x and
        p must not overlap."""
        self._require_real("periodogram")
        t = self._torch
        n = int(self.params.lengths[0])
        m = n // 2
        if t is None or not isinstance(x, t.Tensor) or not isinstance(p, t.Tensor):
            raise invalid_configuration("periodogram takes torch tensors (in, out)")
        if pad not in ("zero", "reflect"):
            raise invalid_configuration("periodogram: pad must be \"zero\" or \"reflect\", got %r" % (pad,))
        if x.dim() not in (1, 2) or x.numel() == 0:
            raise invalid_configuration("periodogram: the in tensor must be 1-D or 2-D (signal, sample) and not empty, got "
                                        "shape %s" % (tuple(x.shape),))
        if p.dim() != x.dim() + 1 or p.numel() == 0:
            raise invalid_configuration("periodogram: the out tensor must be %d-D (%srow, bin) and not empty, got shape %s"
                                        % (x.dim() + 1, "signal, " if x.dim() == 2 else "", tuple(p.shape)))
        for name, a in (("in", x), ("out", p)):
            if a.dtype != self._real_dtype:
                raise invalid_configuration("periodogram: dtype %s of the %s tensor does not match the descriptor (%s real "
                                            "scalars)" % (a.dtype, name, self._scalar))
        if p.shape[-1] != m + 1:
            raise invalid_configuration("periodogram: the out tensor holds %d bins per row, a frame of %d scalars has %d"
                                        % (p.shape[-1], n, m + 1))
        n_x = int(x.shape[0]) if x.dim() == 2 else 1
        n_p = int(p.shape[0]) if p.dim() == 3 else 1
        if n_x != n_p:
            raise invalid_configuration("periodogram: %d input signals but %d output signals" % (n_x, n_p))
        for name, a in (("in", x), ("out", p)):
            if a.stride(-1) != 1 and a.shape[-1] > 1:
                raise invalid_configuration("periodogram: the %s tensor needs unit inner stride, got %d" % (name, a.stride(-1)))
        n_frames, avg = int(n_frames), int(frames_per_row)
        if n_frames < 1:
            raise invalid_configuration("periodogram: n_frames %d, must be at least 1" % n_frames)
        if not 1 <= avg <= n_frames:
            raise invalid_configuration("periodogram: frames_per_row %d, must be in [1, n_frames = %d]" % (avg, n_frames))
        n_rows = (n_frames + avg - 1) // avg
        if int(p.shape[-2]) != n_rows:
            raise invalid_configuration("periodogram: the out tensor holds %d rows, ceil(n_frames %d / frames_per_row %d) is %d"
                                        % (p.shape[-2], n_frames, avg, n_rows))
        in_len = int(x.shape[-1])
        in_pitch = int(x.stride(0)) if x.dim() == 2 and n_x > 1 else in_len
        row_pitch = int(p.stride(-2)) if n_rows > 1 else m + 1
        out_pitch = int(p.stride(0)) if p.dim() == 3 and n_p > 1 else n_rows * row_pitch
        if in_pitch < in_len:
            raise invalid_configuration("periodogram: the signals of the in tensor overlap (stride %d below the length %d)"
                                        % (in_pitch, in_len))
        if row_pitch < m + 1:
            raise invalid_configuration("periodogram: the rows of the out tensor overlap (row stride %d below the %d bins)"
                                        % (row_pitch, m + 1))
        if out_pitch < n_rows * row_pitch:
            raise invalid_configuration("periodogram: the signals of the out tensor overlap (stride %d below %d rows of pitch "
                                        "%d)" % (out_pitch, n_rows, row_pitch))
        hop, lead = int(hop), int(lead)
        if hop < 1:
            raise invalid_configuration("periodogram: hop %d, must be at least 1" % hop)
        if not 0 <= lead < n:
            raise invalid_configuration("periodogram: lead %d, must be in [0, %d)" % (lead, n))
        last = (n_frames - 1) * hop
        if pad == "zero":
            if last >= in_len + lead:
                raise invalid_configuration("periodogram: frame %d starts at sample %d - lead %d, beyond the in_length %d: "
                                            "every frame must hold at least one sample (n_frames, hop)"
                                            % (n_frames - 1, last, lead, in_len))
        else:
            if lead > in_len - 1:
                raise invalid_configuration("periodogram: lead %d above in_length - 1 = %d: reflection mirrors an index at "
                                            "most once" % (lead, in_len - 1))
            if last + n > in_len + 2 * lead:
                raise invalid_configuration("periodogram: frame %d ends at sample %d - lead %d, beyond the signal of "
                                            "in_length %d reflected by lead on both sides (n_frames, hop)"
                                            % (n_frames - 1, last + n, lead, in_len))
        self._require_on_device("periodogram", (("in", x), ("out", p)))
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_periodogram_ex(self._plan, _ptr(x), _ptr(p), n_x, in_len, in_pitch, hop, lead,
                                               _lib.PAD_REFLECT if pad == "reflect" else _lib.PAD_ZERO, n_frames, avg,
                                               row_pitch, out_pitch, n_deps, dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    # -- convolution / correlation of pairs of real rows, GCC-PHAT (every plan of the REAL domain; no reference equivalent) --
    def prepare_pairs(self):
        """Make convolve_pairs() and correlate_pairs() available: resolves the kernels (a length without pre-compiled ones
        is compiled here).  Takes no data and uploads nothing; a second call does nothing (inside a stream capture every call is refused).  A
        copy() shares the result.
        The verbs never prepare on their own.  A length whose two LDS image sets do not fit the device is refused here."""
        self._require_real("prepare_pairs")
        _check(lib.pfft_plan_prepare_pairs(self._plan))
        self._pairs_prepared = True

    def _pairs(self, verb, mode, x, y, out, phat_floor, dependencies, want_event):
        self._require_real(verb)
        if not getattr(self, "_pairs_prepared", False):
            raise invalid_configuration("%s: prepare_pairs missing: the plan was not prepared for pairs of rows "
                                        "(prepare_pairs())" % verb)
        t = self._torch
        n = int(self.params.lengths[0])
        names = (("x", x), ("y", y), ("out", out))
        if t is None or not all(isinstance(a, t.Tensor) for _, a in names):
            raise invalid_configuration("%s takes torch tensors (x, y, out)" % verb)
        for name, a in names:
            if a.dtype != self._real_dtype:
                raise invalid_configuration("%s: dtype %s of the %s tensor does not match the descriptor (%s real scalars)"
                                            % (verb, a.dtype, name, self._scalar))
        for name, a in names:
            if a.dim() not in (1, 2) or a.numel() == 0:
                raise invalid_configuration("%s: the %s tensor must be 1-D or 2-D (row, sample) and not empty, got shape %s"
                                            % (verb, name, tuple(a.shape)))
            if a.shape[-1] > n:
                raise invalid_configuration("%s: the last dimension of the %s tensor is %d, above the descriptor's length %d"
                                            % (verb, name, a.shape[-1], n))
        for name, a in names:
            if a.stride(-1) != 1 and a.shape[-1] > 1:
                raise invalid_configuration("%s: the %s tensor needs unit inner stride, got %d" % (verb, name, a.stride(-1)))
        rows = [int(a.shape[0]) if a.dim() == 2 else 1 for _, a in names]
        if not rows[0] == rows[1] == rows[2]:
            raise invalid_configuration("%s: %d rows of x, %d rows of y, %d rows of out: the row counts must be equal"
                                        % (verb, rows[0], rows[1], rows[2]))
        lengths = [int(a.shape[-1]) for _, a in names]
        pitches = [int(a.stride(0)) if a.dim() == 2 and rows[0] > 1 else length for (_, a), length in zip(names, lengths)]
        for (name, _), pitch, length in zip(names, pitches, lengths):
            if pitch < length:
                raise invalid_configuration("%s: the rows of the %s tensor overlap (stride %d below the length %d)"
                                            % (verb, name, pitch, length))
        floor = 0.0
        if phat_floor is not None:
            floor = float(phat_floor)
            info = t.finfo(self._real_dtype)
            if not (floor > 0.0) or floor == float("inf") or floor < info.tiny or floor > info.max:
                raise invalid_configuration("%s: phat_floor %r must be None (no phase transform) or a positive, finite, "
                                            "normal number of the descriptor's real type (%g ... %g)"
                                            % (verb, phat_floor, info.tiny, info.max))
        self._require_on_device(verb, names)
        dep_arr, n_deps, ev, ev_ref = self._marshal(dependencies, want_event)
        _check(lib.pfft_execute_pairs_ex(self._plan, mode, _ptr(x), _ptr(y), _ptr(out), rows[0], lengths[0], pitches[0],
                                         lengths[1], pitches[1], lengths[2], pitches[2], floor, n_deps, dep_arr, ev_ref))
        return event(ev.value if want_event else None, self)

    def convolve_pairs(self, x, y, out, dependencies=None, want_event=True):
        """Circular convolution of row r of `x` with row r of `y` into row r of `out`, in one kernel launch: both operands
        are data of this call.  `x`, `y`, `out`: (rows, L) or (L,) of the descriptor's real type, unit inner stride, row
        pitch stride(0), equal row counts; the three L may differ and are at most N.  The rows of x and y are extended
        with zeros to N as they are loaded, and the first out.shape[-1] scalars of a result row are stored:
          out[r, l] = c * N * sum_n xe[r, n] * ye[r, (l - n) mod N]  =  c * N * np.fft.irfft(rfft(xe[r]) * rfft(ye[r]))[l]
        with c = forward_scale ** 2 * backward_scale: the backward transform is unnormalised, as in convolve(), and
        backward_scale = 1 / N gives the plain sums.  With x.shape[-1] + y.shape[-1] - 1 <= N nothing aliases and a row
        is c * N * np.convolve(x[r], y[r]) followed by zeros.  `out` must overlap neither input; x and y may be the same."""
        return self._pairs("convolve_pairs", _lib.CONVOLVE, x, y, out, None, dependencies, want_event)

    def correlate_pairs(self, x, y, out, phat_floor=None, dependencies=None, want_event=True):
        """Circular cross-correlation of row r of `x` with row r of `y` into row r of `out`, in one kernel launch; the
        tensors as in convolve_pairs().
          out[r, l] = c * N * sum_n xe[r, (n + l) mod N] * ye[r, n]  =  c * N * np.fft.irfft(rfft(xe[r]) * conj(rfft(ye[r])))[l]
        -- the sign convention of filter(correlate=True), y in the filter's place.  With x.shape[-1] + y.shape[-1] - 1 <= N
        nothing aliases: the lags 0 ... len(x) - 1 stand at out[r, 0 ...] and the lags -1 ... -(len(y) - 1) at out[r, N - 1]
        downwards.  Passing the same tensor as x and y is autocorrelation.
        phat_floor=f > 0 is the generalised cross-correlation with phase transform (GCC-PHAT): every bin P[k] of
        rfft(xe) * conj(rfft(ye)) (unscaled) is divided by max(abs(P[k]), f) and the scale is backward_scale alone:
        out[r] = backward_scale * N * irfft(P / maximum(abs(P), f)).  Bins above the floor keep only their phase; a bin
        below it keeps its magnitude over f, so silence stays silent.  abs(P[k]) is formed without squaring numbers of P's
        magnitude: the branch is right wherever P[k] is a finite, normal number of the descriptor's real type.  argmax(out[r]) is the delay of x against y."""
        return self._pairs("correlate_pairs", _lib.CORRELATE, x, y, out, phat_floor, dependencies, want_event)

    def wait(self):
        """queue.wait(): everything submitted on the plan's stream has finished."""
        _check(lib.pfft_plan_wait(self._plan))
