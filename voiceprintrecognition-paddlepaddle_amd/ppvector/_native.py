"""ctypes binding of libvpmi.so (include/vpmi.h) -- the only compute backend of this package.

There is deliberately NO CPU / PyTorch fallback: if the HIP library is missing or no GPU is
visible, every compute entry point raises.  PyTorch is used for device memory, the current HIP
stream and (later) torch.distributed only.
"""
import ctypes as C
import os
import threading

import torch

from ._abi import parse

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get('VPMI_LIB') or os.path.join(PKG_ROOT, 'lib', 'libvpmi.so')   # VPMI_LIB: A/B a build

c_void_p, c_int, c_float, c_size_t = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# include/vpmi.h is the one statement of the ABI: the struct classes, the VP_* / VPMI_VERSION constants and _PROTOS
# {name: (restype, [argtypes])} below are read from it at import (ppvector/_abi.py, docs/abi_binding.md).  Only the Python names of
# the structs are chosen here; a struct the header adds needs an entry.
STRUCT_CLASSES = {
    'vp_fbank_opts': 'FbankOpts', 'vp_mel_opts': 'MelOpts', 'vp_conv1d_desc': 'Conv1dDesc', 'vp_res2_train_desc': 'Res2TrainDesc',
    'vp_tdnn_layer': 'TdnnLayer', 'vp_se_res2_block': 'SeRes2Block', 'vp_asp_weights': 'AspWeights',
    'vp_ecapa_weights': 'EcapaWeights', 'vp_tdnn_weights': 'TdnnWeights',
    'vp_resblock': 'ResBlock', 'vp_cam_layer': 'CamLayer', 'vp_transit': 'Transit', 'vp_campplus_weights': 'CamppWeights',
    'vp_rse_block': 'RseBlock', 'vp_resnetse_weights': 'ResnetSeWeights',
    'vp_aff_weights': 'AffWeights', 'vp_ere_block': 'EreBlock', 'vp_eres2net_weights': 'Eres2netWeights',
    'vp_r2n_block': 'R2nBlock', 'vp_res2net_weights': 'Res2netWeights',
}
HEADER = os.path.normpath(os.path.join(PKG_ROOT, '..', 'include', 'vpmi.h'))        # the file build.py depends on
with open(HEADER, encoding='utf-8') as _f:
    _hdr = parse(_f.read(), STRUCT_CLASSES)
globals().update(_hdr.consts)
globals().update({cls.__name__: cls for cls in _hdr.structs.values()})
_PROTOS = _hdr.protos

EXPORTED_SYMBOLS = tuple(_PROTOS.keys())

_lib = None
_lock = threading.RLock()      # re-entrant: ctx() -> load_library() nest
_ctx = {}


class VpmiError(RuntimeError):
    pass


def load_library():
    """dlopen libvpmi.so and set the prototypes.  Works without a GPU (symbol checks only)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise VpmiError(f'{LIB_PATH} is missing: build it with `python {PKG_ROOT}/build.py` '
                                '(there is no CPU fallback)')
            dll = C.CDLL(LIB_PATH)
            for name, (res, args) in _PROTOS.items():
                fn = getattr(dll, name)
                fn.restype = res
                fn.argtypes = args
            if dll.vp_version() != VPMI_VERSION:         # a stale build beside a newer header: its argument lists may differ
                raise VpmiError(f'{LIB_PATH} is version {dll.vp_version()}, {HEADER} declares {VPMI_VERSION}: rebuild the library')
            _lib = dll
    return _lib


lib = load_library


def default_device():
    """The current HIP device as a torch.device; raises when none is visible (no CPU fallback)."""
    if not torch.cuda.is_available():
        raise VpmiError('no HIP device visible: the ppvector MI355X engine has no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def _device_index(device):
    """None, an int, a string or a torch.device -> the device's index (the current device where none is named)."""
    if not torch.cuda.is_available():
        raise VpmiError('no HIP device visible: the ppvector MI355X engine has no CPU fallback')
    if device is not None and not isinstance(device, int):
        device = torch.device(device).index
    return torch.cuda.current_device() if device is None else device


def ctx(device=None):
    """Per-device vp_ctx; requires a visible GPU."""
    device = _device_index(device)
    library = lib()
    with _lock:
        if device not in _ctx:
            h = library.vp_create(device)
            if not h:
                raise VpmiError(f'vp_create({device}) failed')
            _ctx[device] = h
            # the grid-barrier words of the fused training kernels live in a tensor of OURS (csrc/api.hip: vp_set_grid_barrier_words): the
            # data-parallel step all-reduces the bail-out flag with the gradients and polls it with an asynchronous copy (train/step.py)
            # (never under a stream capture: an allocation + synchronise there would break it; the context then keeps its own words, which
            # work the same on one rank -- only the collective drop across ranks needs the tensor)
            if not torch.cuda.is_current_stream_capturing():
                words = torch.zeros(GRID_WORDS, dtype=torch.int32, device=torch.device('cuda', device))
                torch.cuda.synchronize(device)
                if library.vp_set_grid_barrier_words(h, words.data_ptr()) == 0:
                    _grid_words[device] = words
    return _ctx[device]


GRID_WORDS, FAULT_WORD = 512, 8 * 32 + 1       # csrc/common.h: VP_FAULT_WORD
_grid_words = {}


def grid_words(device=None):
    """The context's grid-barrier words as an int32 tensor (512,) -- element FAULT_WORD is the bail-out flag -- or None."""
    ctx(device)
    return _grid_words.get(_device_index(device))


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


# Kernels that write parameters or buffers through raw pointers (the flat Adam step, the BatchNorm running statistics of a
# train-mode forward) do not move torch's per-tensor version counters.  Every such writer bumps this epoch; caches of packed
# weights (ppvector/models/engine.py) carry it in their key.
_weights_epoch = 0


def bump_weights_epoch():
    global _weights_epoch
    _weights_epoch += 1


def weights_epoch():
    return _weights_epoch


def check(rc, c=None):
    if rc != 0:
        msg = lib().vp_last_error(c).decode('utf-8', 'replace') if c else ''
        raise VpmiError(f'libvpmi error {rc}: {msg}')


def ptr(t):
    return None if t is None else t.data_ptr()


def dtype_id(torch_dtype):
    if torch_dtype == torch.float32:
        return VP_F32
    if torch_dtype == torch.bfloat16:
        return VP_BF16
    raise VpmiError(f'unsupported dtype {torch_dtype}')


class Workspace:
    """Grow-only device scratch, one per consumer; reused across calls so the steady state
    allocates nothing (hipGraph-friendly)."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes, device):
        # one buffer per (device, stream): the same consumer may run on several streams at once (engine.forward_streams' shard
        # tails), and a kernel's scratch must not be shared between launch sequences that overlap
        key = (device, torch.cuda.current_stream(device).cuda_stream if device.type == 'cuda' else 0)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf
