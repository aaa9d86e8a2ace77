"""The hash field's SDF with its gradient in the point, differentiable in the parameters (include/lab4d_hashsdf.h, csrc/hashsdf.hip):
what compute_gradient(..., create_graph=True) (utils/torch_utils.py:4-27) gives the positional-encoding fields, for the field whose
encoding has no double backward.  One autograd Function over the two calls: the forward returns sdf and grad01 = d sdf / d x01, the
backward takes cotangents on BOTH and returns the gradients of the table and of the geometry net in closed form (second-order terms
included).  The rules are written down in the header and in csrc/hashsdf_math.hpp.  Nothing here synchronises with the host, and the
calls can be captured in a hipGraph (see sdf_grad01 for what a capture of the backward needs)."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib

ENC, HID = 32, 64
ROW = HID * ENC + HID + HID + 1  # one partial row of the dense gradients: dW1 | db1 | dw2 | db2 (include/lab4d_hashsdf.h, WORK)
MAX_ROWS = 512                   # LAB4D_HASHSDF_WORK_ROWS: the largest resident grid of the adjoint
_WORK = {}


def work_buffer(device):
    """The default work buffer of the adjoint's dense gradients, (MAX_ROWS, ROW) float32 (4.5 MB), one per device, allocated on first
    use and kept.  Every call writes the rows it reads, nothing is cleared.  It is shared by every call on the device: code that runs
    backward passes on SEVERAL streams at once passes a buffer of its own per stream (the `work` argument of sdf_grad01).
    It has to exist BEFORE a hipGraph capture (an eager warm-up call, or this function): a buffer born in a graph's private pool must
    not be kept in a module global and touched by eager calls; inside a capture a missing buffer is an error."""
    key = torch.device(device)
    if key.index is None:
        key = torch.device(key.type, torch.cuda.current_device())
    if key not in _WORK:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("lab4d_amd.hashsdf: the work buffer does not exist yet: call hashsdf.work_buffer(device), or run one eager "
                               "forward + backward, before capturing")
        _WORK[key] = torch.empty(MAX_ROWS, ROW, dtype=torch.float32, device=key)
    return _WORK[key]


def _check(x01, table, res, log2_T, W1, b1, w2, b2, work_rows):
    for name, t in (("x01", x01), ("table", table), ("res", res), ("W1", W1), ("b1", b1), ("w2", w2), ("b2", b2)):
        if not torch.is_tensor(t):
            raise RuntimeError("lab4d_amd.hashsdf: %s must be a device tensor, got %s" % (name, type(t).__name__))
    if x01.requires_grad:
        raise RuntimeError("lab4d_amd.hashsdf: the points must not require grad: second derivatives in x are not implemented "
                           "(pass xyz.detach(); the gradients go to the table and the geometry net)")
    if x01.dtype != torch.float32 or x01.ndim != 2 or x01.shape[1] != 3:
        raise RuntimeError("lab4d_amd.hashsdf: x01 must be float32 (S, 3), got %s %s" % (x01.dtype, tuple(x01.shape)))
    if x01.shape[0] >= 1 << 31:
        raise RuntimeError("lab4d_amd.hashsdf: %d points, must be below 2^31" % x01.shape[0])
    if table.dtype != torch.float32 or table.ndim != 3:
        raise RuntimeError("lab4d_amd.hashsdf: table must be float32 (L, 2^log2_T, F), got %s %s" % (table.dtype, tuple(table.shape)))
    L, T, F = table.shape
    log2_T = int(log2_T)
    if L * F != ENC or L > 32 or F > 8:
        raise RuntimeError("lab4d_amd.hashsdf: L = %d, F = %d: the geometry net is instantiated for L * F = 32 hash features (L <= 32, F <= 8)" % (L, F))
    if not 4 <= log2_T <= 24 or T != 1 << log2_T:
        raise RuntimeError("lab4d_amd.hashsdf: table has %d rows per level, log2_T = %d must lie in [4, 24] with 2^log2_T rows" % (T, log2_T))
    if res.dtype != torch.int32 or res.numel() != L:
        raise RuntimeError("lab4d_amd.hashsdf: res must be int32 (L = %d,), got %s %s" % (L, res.dtype, tuple(res.shape)))
    for name, t, shape in (("W1", W1, (HID, ENC)), ("b1", b1, (HID,)), ("w2", w2, (HID,)), ("b2", b2, (1,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise RuntimeError("lab4d_amd.hashsdf: %s must be float32 %s, got %s %s" % (name, shape, t.dtype, tuple(t.shape)))
    if work_rows is not None and not 1 <= int(work_rows) <= MAX_ROWS:
        raise RuntimeError("lab4d_amd.hashsdf: work_rows = %d outside [1, %d]" % (int(work_rows), MAX_ROWS))
    _lib.require_device(x01, table, res, W1, b1, w2, b2)


class _HashSdf(Function):
    @staticmethod
    def forward(ctx, x01, table, res, log2_T, W1, b1, w2, b2, work_rows, work):
        ctx.set_materialize_grads(False)  # an output nothing depends on arrives as None and reaches the library as a NULL cotangent
        x01, table, W1, b1, w2, b2 = (t.detach().contiguous() for t in (x01, table, W1, b1, w2, b2))
        res = res.contiguous()
        S, (L, _, F) = x01.shape[0], table.shape
        sdf = torch.empty(S, dtype=torch.float32, device=x01.device)
        grad01 = torch.empty(S, 3, dtype=torch.float32, device=x01.device)
        # algorithmic bytes: the table gathered twice (8 vertices x F floats per level), the point read, 4 floats written
        with _lib.timed("k_hashsdf_fwd", (2.0 * S * (2 * HID * ENC), 4.0 * S * (2 * 8 * L * F + 3 + 4))):
            _lib.call("hashsdf_forward", x01, table, res, S, L, log2_T, F, W1, b1, w2, b2, sdf, grad01)
        ctx.save_for_backward(x01, table, res, W1, b1, w2, b2)
        ctx.log2_T, ctx.work_rows, ctx.work = log2_T, work_rows, work
        if work is None and any(ctx.needs_input_grad[i] for i in (4, 5, 6, 7)):
            work_buffer(x01.device)  # (allocated here on the first eager call; a capture without it is refused before the backward)
        return sdf, grad01

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sdf, g_grad01):
        if g_sdf is None and g_grad01 is None:  # nothing depends on either output
            return (None,) * 10
        x01, table, res, W1, b1, w2, b2 = ctx.saved_tensors
        S, (L, _, F) = x01.shape[0], table.shape
        need = ctx.needs_input_grad
        g_table = torch.zeros_like(table) if need[1] else None
        g_W1 = torch.empty_like(W1) if need[4] else None
        g_b1 = torch.empty_like(b1) if need[5] else None
        g_w2 = torch.empty_like(w2) if need[6] else None
        g_b2 = torch.empty_like(b2) if need[7] else None
        dense = any(g is not None for g in (g_W1, g_b1, g_w2, g_b2))
        if g_table is None and not dense:
            return (None,) * 10
        g_sdf = g_sdf.contiguous().float() if g_sdf is not None else None
        g_grad01 = g_grad01.contiguous().float() if g_grad01 is not None else None
        work = (ctx.work if ctx.work is not None else work_buffer(x01.device)) if dense else None
        rows = int(ctx.work_rows) if ctx.work_rows is not None else MAX_ROWS
        with _lib.timed("k_hashsdf_bwd", (2.0 * S * (3 * HID * ENC), 4.0 * S * (2 * 8 * L * F + 3 + 4))):
            _lib.call("hashsdf_backward", x01, table, res, S, L, ctx.log2_T, F, W1, b1, w2, b2, g_sdf, g_grad01, g_table, g_W1, g_b1, g_w2, g_b2, work, rows)
        return None, g_table, None, None, g_W1, g_b1, g_w2, g_b2, None, None


def sdf_grad01(x01, table, res, log2_T, W1, b1, w2, b2, work_rows=None, work=None):
    """x01 (S,3) float32 box coordinates (must NOT require grad), table (L, 2^log2_T, F) with L * F = 32, res (L,) int32 device tensor,
    W1 (64,32), b1 (64): the geometry net's first Linear, w2 (64), b2 (1): row 0 of its head
    -> sdf (S,), grad01 (S,3) = d sdf / d x01 (zero outside [0,1]^3, where sdf = w2 . relu(b1) + b2).
    Both outputs are differentiable in table, W1, b1, w2 and b2; only the gradients that are needed are computed.
    work_rows: the resident grid of the adjoint = the number of partial rows its dense gradients are folded from (default: 512); the
    dense gradients are deterministic for a given value.
    work: a float32 device buffer of at least work_rows * 2177 elements for the adjoint's partial rows (one per stream, for callers that
    run backward passes on several streams at once); default: work_buffer(device), shared by every call on the device.
    Graph capture: forward and backward neither read back nor allocate besides their outputs.  A capture of the backward follows
    torch's rule for capturing autograd work: warm up on a side stream, and keep no autograd graph of an eager call alive across the
    capture.  A kept eager graph keeps the parameters' AccumulateGrad nodes, which are bound to the stream they were made on; reused
    inside the capture, the engine orders the capture stream against that stream with an event, which drags it (the legacy default
    stream, after a plain eager call) into the capture, and closing such a capture takes the HIP runtime down."""
    _check(x01, table, res, log2_T, W1, b1, w2, b2, work_rows)
    if work is not None:
        rows = MAX_ROWS if work_rows is None else int(work_rows)
        if not torch.is_tensor(work) or work.dtype != torch.float32 or not work.is_cuda or not work.is_contiguous() or work.numel() < rows * ROW:
            raise RuntimeError("lab4d_amd.hashsdf: work must be a contiguous float32 device tensor of at least work_rows * %d = %d elements" % (ROW, rows * ROW))
    return _HashSdf.apply(x01, table, res, int(log2_T), W1, b1, w2, b2, None if work_rows is None else int(work_rows), work)
