"""3x3 convolution / deformable convolution forward as one fp32-MFMA implicit GEMM (csrc/conv_igemm.hip), and the
one-pass bias / ReLU backward of every conv + bias [+ ReLU] (csrc/frozen_bn.hip: jdet_bias_act_backward).

Replaces the `nn.Conv(3x3) [+ ReLU]` of ConvModule (python/jdet/models/utils/modules.py:L91-175) in the head towers,
the FPN and the RPNs, and -- where no gradient is needed -- the im2col + matmul pair of DeformConv.execute
(python/jdet/ops/dcn_v1.py:L412-454): no column matrix, bias / ReLU / gap-row mask applied to the accumulators.  The
kernel is a forward kernel: `_ConvBiasAct` gives it a backward through the library's data / weight gradient kernels
(the ReLU mask and the bias gradient come out of one pass over the incoming gradient); the training path of the
deformable conv keeps the column matrix, which its weight-gradient GEMM reads.

Measured on MI355X, 256 -> 256 channels, batch 2 (scripts/conv_igemm_timing.py, profiles/r03_conv_igemm.md):
128^2 map 296 us (130.6 TFLOP/s, MFMA busy 80.8 %) vs 394 us for library conv + bias + ReLU; 64^2 map 86-94 vs 126 us;
32^2 / 16^2 / 8^2 maps 37 / 18 / 16 us vs 55 / 29 / 26 us (K steps split over workgroups through a scratch buffer).

The big shapes (at least 512 tiles of 128 x 128, Cin % 32 == 0: the P3 layers of the 1024^2 step) go to
csrc/conv_bf16x3.hip instead: the same convolution on the bf16 matrix pipe through an exact three-way split of the fp32
operands, as accurate as the fp32 kernel; see BF16X3 below and profiles/conv_bf16x3.md.
"""
import os
import weakref

import torch

from jdet_amd import _lib as L


def supported(cin, cout):
    return bool(L.lib().jdet_conv3x3_igemm_supported(int(cin), int(cout)))


def weight_krsc(weight):
    """(Cout, Cin, 3, 3) logical -> (Cout, 3, 3, Cin) contiguous fp32; free when the weight is channels_last"""
    return L.f32c(weight.permute(0, 2, 3, 1))


def _plain_conv(conv):
    """a plain nn.Conv2d (zeros padding, given as numbers) called outside autocast"""
    return (type(conv).__name__ == "Conv2d" and conv.padding_mode == "zeros" and not isinstance(conv.padding, str)
            and not torch.is_autocast_enabled())


def _fits_32bit(positions, cin, cout, pad=0):
    """the kernels address with 32-bit byte offsets (`pad`: rows a kernel may address past the map)"""
    return (positions + pad) * max(cin, cout) < 2 ** 30


def _check_shapes(N, H, W, Cin, w_krsc=None, offset=None):
    """the weight (Cout,3,3,Cin) matches x (N,H,W,Cin); the offset is (N,18,H,W)"""
    if w_krsc is not None and w_krsc.shape[1:] != (3, 3, Cin):
        raise ValueError("weight %r does not match input channels %d" % (tuple(w_krsc.shape), Cin))
    if offset is not None and tuple(offset.shape) != (N, 18, H, W):
        raise ValueError("offset must be (N, 18, H, W), got %r" % (tuple(offset.shape),))


# The big dense layers on the bf16 matrix pipe through an exact three-way split of the fp32 operands (csrc/conv_bf16x3.hip,
# profiles/conv_bf16x3.md): the shapes the fp32 kernel gives its 128 x 128 tile (at least 512 of them) with Cin % 32 == 0,
# automatic tile, plain form -- with and without gradients alike (one kernel per shape: the no-grad route of a layer
# computes what its training forward computes).  JDET_CONV_BF16X3 switches the forward route, JDET_CONV_BF16X3_DGRAD the
# data gradient of the same layers (grad_x = this kernel on the flipped weights, in place of the library's); the defaults
# follow the step pairs of profiles/conv_bf16x3.md.
BF16X3 = os.environ.get("JDET_CONV_BF16X3", "1") == "1"
BF16X3_DGRAD = os.environ.get("JDET_CONV_BF16X3_DGRAD", "1") == "1"


def bf16x3_supported(cin, cout):
    return bool(L.lib().jdet_conv3x3_bf16x3_supported(int(cin), int(cout)))


def bf16x3_big(positions, cin, cout):
    """the shapes the split kernel is routed to: conv_igemm.hip's `big` rule (128 x 128 tiles >= 512), channels it takes"""
    # (plain integer tests first: every fused 3x3 call of every model passes here, most of them below the rule)
    if ((positions + 127) // 128) * ((cout + 127) // 128) < 512 or cin % 32 != 0 or not _fits_32bit(positions, cin, cout):
        return False
    return bf16x3_supported(cin, cout)


def conv3x3_bf16x3_nhwc(x_nhwc, w_krsc, bias=None, relu=False, rowmask=None):
    """x_nhwc (N,H,W,Cin) contiguous fp32, w_krsc (Cout,3,3,Cin) -> (N,H,W,Cout) by jdet_conv3x3_bf16x3_forward (any
    shape it supports; `conv3x3_nhwc` routes the big ones here)"""
    L.need_device(x_nhwc, w_krsc, bias, rowmask)
    N, H, W, Cin = x_nhwc.shape
    Cout = w_krsc.shape[0]
    _check_shapes(N, H, W, Cin, w_krsc)
    x_nhwc, w_krsc = L.f32c(x_nhwc), L.f32c(w_krsc)
    y = torch.empty((N, H, W, Cout), dtype=torch.float32, device=x_nhwc.device)
    L.check(L.lib().jdet_conv3x3_bf16x3_forward(
        L.ptr(x_nhwc), N, H, W, Cin, L.ptr(w_krsc), Cout, L.ptr(L.f32c(bias)) if bias is not None else None,
        int(bool(relu)), L.ptr(L.f32c(rowmask)) if rowmask is not None else None, L.ptr(y), L.stream_ptr(x_nhwc)),
        "jdet_conv3x3_bf16x3_forward")
    return y


def conv3x3_nhwc(x_nhwc, w_krsc, bias=None, relu=False, rowmask=None, offset=None, tile=0, bf16x3=None):
    """x_nhwc (N,H,W,Cin) contiguous fp32, w_krsc (Cout,3,3,Cin), offset (N,18,H,W) or None -> (N,H,W,Cout).
    bf16x3: None = the JDET_CONV_BF16X3 route for big shapes, True / False = that route forced on / off (it never
    applies to a forced tile or the deformable form)"""
    L.need_device(x_nhwc, w_krsc, bias, rowmask, offset)
    N, H, W, Cin = x_nhwc.shape
    Cout = w_krsc.shape[0]
    _check_shapes(N, H, W, Cin, w_krsc, offset)
    if (BF16X3 if bf16x3 is None else bf16x3) and tile == 0 and offset is None and bf16x3_big(N * H * W, Cin, Cout):
        return conv3x3_bf16x3_nhwc(x_nhwc, w_krsc, bias, relu, rowmask)
    x_nhwc, w_krsc = L.f32c(x_nhwc), L.f32c(w_krsc)
    y = torch.empty((N, H, W, Cout), dtype=torch.float32, device=x_nhwc.device)
    ws, nbytes = None, 0
    if tile == 0 and offset is None:      # small maps: K split over workgroups through a scratch buffer
        nbytes = L.lib().jdet_conv3x3_igemm_workspace(N, H, W, Cin, Cout)
        if nbytes:
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=x_nhwc.device)
    L.check(L.lib().jdet_conv3x3_igemm_forward(
        L.ptr(x_nhwc), N, H, W, Cin, L.ptr(w_krsc), Cout,
        L.ptr(L.f32c(bias)) if bias is not None else None, int(bool(relu)),
        L.ptr(L.f32c(rowmask)) if rowmask is not None else None,
        L.ptr(L.f32c(offset)) if offset is not None else None,
        int(tile), L.ptr(y), L.ptr(ws), nbytes, L.stream_ptr(x_nhwc)), "jdet_conv3x3_igemm_forward")
    return y


def conv3x3(x, weight, bias=None, relu=False, offset=None, tile=0):
    """NCHW-logical convenience form: returns a channels_last (N, Cout, H, W) tensor"""
    y = conv3x3_nhwc(L.f32c(x.permute(0, 2, 3, 1)), weight_krsc(weight), bias, relu, None, offset, tile)
    return y.permute(0, 3, 1, 2)


# smallest map (positions = N*H*W) the fused path takes: it measured faster than library conv + bias + ReLU at every
# size once small maps split their K steps over workgroups; the deformable form only where it beats im2col + GEMM
MIN_POSITIONS = int(os.environ.get("JDET_CONV_MIN_POS", "1"))
DEFORM_MIN_POSITIONS = 32768
ENABLED = os.environ.get("JDET_CONV_IGEMM", "1") == "1"     # A/B switch for measurements
# Train step: the fused forward with a backward of its own (`_ConvBiasAct`).  S2ANet step 30.05 ms with it, 30.37 ms
# without (two A/B pairs, profiles/r03_conv_igemm.md); JDET_CONV_IGEMM_TRAIN=0 switches it off.
TRAIN = os.environ.get("JDET_CONV_IGEMM_TRAIN", "1") == "1"


def needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def preferred(x, weight, min_positions=None):
    """x (N, Cin, H, W) logical, weight (Cout, Cin, 3, 3): is the fused kernel the faster choice for this call?"""
    if not (ENABLED and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4):
        return False
    N, Cin, H, W = x.shape
    if tuple(weight.shape[1:]) != (Cin, 3, 3) or not supported(Cin, weight.shape[0]):
        return False
    if not _fits_32bit(N * H * W, Cin, weight.shape[0]):
        return False
    return N * H * W >= (MIN_POSITIONS if min_positions is None else min_positions)


def wgrad_supported(cin, cout):
    return bool(L.lib().jdet_conv3x3_wgrad_supported(int(cin), int(cout)))


def conv3x3_wgrad_nhwc(x_nhwc, gy_nhwc, offset=None, out=None, ksplit=0, rows=None):
    """x (N,H,W,Cin), gy (N,H,W,Cout) contiguous fp32 [offset (N,18,H,W): the deformable form] -> the weight gradient
    (Cout,3,3,Cin).  `out`: a contiguous (Cout,3,3,Cin) buffer the gradient is ADDED to (csrc/conv_wgrad.hip), else a
    fresh zero-filled one.  `rows`: (int32 device list of the non-zero rows of gy, device address of its count) -- the
    sum then runs over those rows only (csrc/conv_rows.hip: jdet_conv3x3_wgrad_rows; plain form)."""
    L.need_device(x_nhwc, gy_nhwc, offset, out)
    N, H, W, Cin = x_nhwc.shape
    Cout = gy_nhwc.shape[3]
    if tuple(gy_nhwc.shape[:3]) != (N, H, W):
        raise ValueError("gy %r does not match x %r" % (tuple(gy_nhwc.shape), tuple(x_nhwc.shape)))
    _check_shapes(N, H, W, Cin, None, offset)
    x_nhwc, gy_nhwc = L.f32c(x_nhwc), L.f32c(gy_nhwc)
    if out is None:
        out = torch.zeros((Cout, 3, 3, Cin), dtype=torch.float32, device=x_nhwc.device)
    elif tuple(out.shape) != (Cout, 3, 3, Cin) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous fp32 (Cout, 3, 3, Cin) tensor")
    L.check(_wgrad_call(x_nhwc, gy_nhwc, offset, N, H, W, Cin, Cout, L.ptr(out), ksplit, rows), "jdet_conv3x3_wgrad")
    return out


def conv3x3_wgrad(x, gy, offset=None, ksplit=0):
    """NCHW-logical form: x (N,Cin,H,W), gy (N,Cout,H,W) -> (Cout,Cin,3,3) logical weight gradient (channels_last
    memory: a view of the kernel's (Cout,3,3,Cin) result)"""
    gw = conv3x3_wgrad_nhwc(L.f32c(x.permute(0, 2, 3, 1)), L.f32c(gy.permute(0, 2, 3, 1)), offset, None, ksplit)
    return gw.permute(0, 3, 1, 2)


# Weight gradient of the igemm layers by csrc/conv_wgrad.hip, on by default; JDET_CONV_WGRAD=0 selects the library's, which
# the shapes `wgrad_supported` refuses take in any case.  Several uses of ONE weight inside one backward pass (a tower
# shared by the pyramid levels) accumulate into the buffer the first use returned: the kernel adds in place, so the engine
# neither zero-fills per call nor sums the uses afterwards.  In the S2ANet step the own kernel measures 26.075 against the
# library's 26.173 ms with 744 -> 727 launches (18 library zero fills and 8 accumulation adds fewer:
# profiles/r06_conv_prefetch.md); the kernel in isolation is in profiles/r04_conv_wgrad.md.
WGRAD = os.environ.get("JDET_CONV_WGRAD", "1") == "1"


def _wgrad_call(x_nhwc, gy_nhwc, offset, N, H, W, Cin, Cout, out_ptr, ksplit, rows=None):
    if rows is not None:
        if offset is not None:
            raise ValueError("the row list belongs to the plain form")
        return L.lib().jdet_conv3x3_wgrad_rows(L.ptr(x_nhwc), L.ptr(gy_nhwc), L.ptr(rows[0]), rows[1], N, H, W, Cin, Cout,
                                               out_ptr, L.stream_ptr(x_nhwc))
    return L.lib().jdet_conv3x3_wgrad(L.ptr(x_nhwc), L.ptr(gy_nhwc), L.ptr(L.f32c(offset)) if offset is not None else None,
                                      N, H, W, Cin, Cout, out_ptr, int(ksplit), L.stream_ptr(x_nhwc))


# weight.data_ptr() -> (backward pass id, device pointer of the (Cout,3,3,Cin) buffer or None = no longer shared, its shape, stream)
_GW_ACC = {}


def shared_wgrad(weight, x_nhwc, gy_nhwc, offset=None, rows=None):
    """weight gradient of y = conv3x3(x, weight) [deformable with `offset`; `rows`: see conv3x3_wgrad_nhwc -- dense and
    row-list uses of one weight share the buffer like any others] for this use of `weight`, as autograd wants
    it: the first use in a backward pass returns a fresh (Cout, Cin, 3, 3) tensor (channels_last memory, so a
    channels_last parameter takes it without a copy); later uses add into that tensor's memory and return None -- until
    a use on another stream returns a tensor of its own: from then on every use of the pass does.  Only the pointer is
    remembered -- a second reference would make AccumulateGrad clone the gradient instead of taking it."""
    tid = torch._C._current_graph_task_id()
    key = weight.data_ptr()          # (the saved tensor may come back in a new Python wrapper: the storage names the weight)
    Cout, Cin = weight.shape[0], weight.shape[1]
    hit = _GW_ACC.get(key)
    # sharing is per STREAM: a use replayed on another stream (the packed levels' side stream) must not add into a
    # buffer whose hand-over to AccumulateGrad the engine orders only against the first use's stream -- it gets its own
    # gradient tensor and autograd adds the two (advisor finding, round 4)
    stream = torch.cuda.current_stream(x_nhwc.device).cuda_stream if x_nhwc.is_cuda else 0
    if tid >= 0 and hit is not None and hit[0] == tid and hit[2] == (Cout, Cin, x_nhwc.device):
        if hit[1] is not None and hit[3] == stream:
            N, H, W, _ = x_nhwc.shape
            x_nhwc, gy_nhwc = L.f32c(x_nhwc), L.f32c(gy_nhwc)
            L.check(_wgrad_call(x_nhwc, gy_nhwc, offset, N, H, W, Cin, Cout, hit[1], 0, rows), "jdet_conv3x3_wgrad")
            return None
        # a second tensor goes to the engine, which is free to add the two OUT OF PLACE and release the first use's
        # buffer: the pointer is dead for the rest of this pass, every later use returns a tensor of its own
        # (tests/test_gpu_conv_routes.py, case 19/side1: a use on the first stream AFTER one on the side stream added
        # into memory the allocator had handed out again -- the next data gradient read an overwritten input)
        _GW_ACC[key] = (tid, None, hit[2], hit[3])
    buf = conv3x3_wgrad_nhwc(x_nhwc, gy_nhwc, offset, rows=rows)
    if tid >= 0 and (_GW_ACC.get(key) is None or _GW_ACC[key][0] != tid):
        _GW_ACC[key] = (tid, buf.data_ptr(), (Cout, Cin, x_nhwc.device), stream)
    return buf.permute(0, 3, 1, 2)


class _WeightRef:
    """what conv_bn.DgradBank reads of a "convolution": its weight (held weakly: the bank must not keep a model alive)"""

    def __init__(self, w):
        self.ref = weakref.ref(w)

    @property
    def weight(self):
        return self.ref()


_DGRAD_BANKS = {}      # device -> {"items": {id(weight): _WeightRef}, "bank": DgradBank}


def dgrad_weight(weight):
    """(Cout, Cin, 3, 3) -> (Cin, 3, 3, Cout) contiguous with the taps flipped: grad_x = conv3x3(grad_y, this).  The
    channels-last fp32 weights seen so far on a device live in ONE bank (conv_bn.DgradBank: one launch rewrites all of
    them -- the per-weight flip + copy pair was 2 launches x 19 weights per S2ANet step), refreshed ONCE PER BACKWARD
    PASS whatever the version counters say -- the fused multi-tensor SGD step (optims/optimizer.py) updates parameters
    without moving `_version` -- and on every call outside a backward pass.  Under graph capture the flip is part of the
    captured pass and its result lives in the graph's pool: nothing a replay reads can be freed or go stale outside it.
    Weights of another layout or dtype, or off the device, take the per-weight form, recomputed on every call."""
    if (not weight.is_cuda or weight.dtype != torch.float32 or not weight.permute(0, 2, 3, 1).is_contiguous()
            or torch.cuda.is_current_stream_capturing()):
        return weight.detach().flip(2, 3).permute(1, 2, 3, 0).contiguous()
    from jdet_amd.ops.conv_bn import DgradBank
    st = _DGRAD_BANKS.setdefault(weight.device, {"items": {}, "bank": None})
    it = st["items"].get(id(weight))
    if it is None or it.weight is not weight or any(v.weight is None for v in st["items"].values()):
        live = {k: v for k, v in st["items"].items() if v.weight is not None}
        it = live[id(weight)] = _WeightRef(weight)
        st["items"] = live
        st["bank"] = DgradBank(list(live.values()))
    # `get` builds the bank's buffer and refreshes it if a version or pointer moved; where it did, the first call of a
    # pass rewrites the bank a second time (one launch, on the passes after a bank was built or a version moved)
    wd = st["bank"].get(it)
    tid = torch._C._current_graph_task_id()
    if tid < 0 or st.get("pass") != tid:
        st["bank"].refresh()
        st["pass"] = tid
    return wd


# bias [+ ReLU] backward as ONE pass (csrc/frozen_bn.hip: jdet_bias_act_backward) instead of the framework's
# threshold_backward + per-channel reduce pair; JDET_BIAS_ACT_BWD=0 switches back (A/B: profiles/r03_conv_igemm.md).
BIAS_ACT_BWD = os.environ.get("JDET_BIAS_ACT_BWD", "1") == "1"
_BWD_WS = {}


def _scratch(cache, nbytes, device):
    """at least `nbytes` (and at least 1) bytes of scratch for the current stream of `device`: in eager mode from `cache`,
    one buffer of at least 1 MiB per (device, stream) that the next call on the stream reuses"""
    if torch.cuda.is_current_stream_capturing():
        # the address is baked into the graph: scratch from the capturing graph's own pool, never from (or into) the
        # cache -- an evicted cache entry would leave replays writing partial sums to freed memory
        return torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        while len(cache) >= 8:       # streams come and go: keep the scratch cache bounded (oldest entry out)
            cache.pop(next(iter(cache)))
        ws = cache[key] = torch.empty((max(nbytes, 1 << 20),), dtype=torch.uint8, device=device)
    return ws


def _bias_bwd_supported(c):
    q = c // 4
    return c % 4 == 0 and ((q <= 256 and 256 % q == 0) or 256 < q <= 1024)


def bias_act_backward(g, y, relu):
    """g, y (N, C, H, W) logical -> (grad of the pre-activation (same logical shape, channels_last), grad_bias (C,)):
    grad_pre = g * [y > 0] when relu, else g itself; grad_bias = grad_pre.sum((0, 2, 3))."""
    N, C, H, W = g.shape
    if (BIAS_ACT_BWD and not relu and g.is_cuda and g.dtype == torch.float32 and not _bias_bwd_supported(C)
            and C <= 256 and N * H * W > 0):
        # channel counts off the vector kernels' grid (the heads' 15- / 5-channel output convs): the any-C column sum
        # (csrc/frozen_bn.hip: jdet_channel_sum) instead of the framework's per-channel reduce (25-60 us per call)
        gn = L.f32c(g.permute(0, 2, 3, 1))
        P = N * H * W
        nbytes = L.lib().jdet_channel_sum_workspace(P, C)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=g.device)
        gb = torch.empty((C,), dtype=torch.float32, device=g.device)
        L.check(L.lib().jdet_channel_sum(L.ptr(gn), P, C, L.ptr(gb), L.ptr(ws), nbytes, L.stream_ptr(gn)),
                "jdet_channel_sum")
        return g, gb
    if not (BIAS_ACT_BWD and g.is_cuda and g.dtype == torch.float32 and _bias_bwd_supported(C) and N * H * W > 0):
        gp = torch.ops.aten.threshold_backward(g, y, 0) if relu else g
        return gp, gp.sum((0, 2, 3))
    gn = L.f32c(g.permute(0, 2, 3, 1))
    P = N * H * W
    nbytes = L.lib().jdet_frozen_bn_act_backward_workspace(P, C)
    ws = _scratch(_BWD_WS, nbytes, g.device)
    gb = torch.empty((C,), dtype=torch.float32, device=g.device)
    gp = torch.empty_like(gn) if relu else gn
    yn = L.f32c(y.permute(0, 2, 3, 1)) if relu else None
    L.check(L.lib().jdet_bias_act_backward(L.ptr(gn), L.ptr(yn), P, C, int(bool(relu)), L.ptr(gp) if relu else None,
                                           L.ptr(gb), L.ptr(ws), ws.numel(), L.stream_ptr(gn)),
            "jdet_bias_act_backward")
    return gp.permute(0, 3, 1, 2), gb


# Row-sparse backward of the regression towers (csrc/conv_rows.hip, profiles/conv_rows.md): a layer whose ConvModule
# carries `row_sparse_grad` takes its data and weight gradients from the non-zero rows of the incoming gradient.  The flag
# is a routing hint only: any gradient is computed correctly, a dense one just slower.  JDET_CONV_ROWS=0: the dense
# kernels (A/B).
ROWS = os.environ.get("JDET_CONV_ROWS", "1") == "1"
_ROWS_WS = {}          # (a cache of its own: the lists `rows_nonzero` returns outlive the next node's bias pass)


def wgrad_rows_workers(cin, cout):
    """how many workgroups at most add a partial sum to one element of gw per call (jdet_conv3x3_wgrad_rows_workers)"""
    return int(L.lib().jdet_conv3x3_wgrad_rows_workers(int(cin), int(cout)))


def rows_supported(cin, cout):
    return bool(L.lib().jdet_conv3x3_rows_supported(int(cin), int(cout)))


def rows_nonzero(g_nhwc, scratch=None):
    """g (N,H,W,C) contiguous fp32 -> (flags (P,) uint8, rows (P,) int32, rows_dilated (P,) int32, counts (2,) int32):
    the rows of g that hold anything but +-0, ascending, and their 3x3 dilation inside each image; list entries past
    their count are -1.  Everything stays on the device (csrc/conv_rows.hip: jdet_rows_nonzero).  The four
    results are views of ONE scratch buffer that the next call on this stream reuses."""
    L.need_device(g_nhwc)
    N, H, W, C = g_nhwc.shape
    P = N * H * W
    g_nhwc = L.f32c(g_nhwc)
    wsb = L.lib().jdet_rows_nonzero_workspace(N, H, W)
    total = 8 * P + 16 + wsb + P            # rows | rows_dilated | counts (padded to 16) | workspace (16 n) | flags
    buf = _scratch(_ROWS_WS, total, g_nhwc.device) if scratch is None else scratch
    rows = buf[:4 * P].view(torch.int32)
    drows = buf[4 * P:8 * P].view(torch.int32)
    counts = buf[8 * P:8 * P + 8].view(torch.int32)
    ws = buf[8 * P + 16:8 * P + 16 + wsb]
    flags = buf[8 * P + 16 + wsb:total]
    L.check(L.lib().jdet_rows_nonzero(L.ptr(g_nhwc), N, H, W, C, L.ptr(flags), L.ptr(rows), L.ptr(drows), L.ptr(counts),
                                      L.ptr(ws), wsb, L.stream_ptr(g_nhwc)), "jdet_rows_nonzero")
    return flags, rows, drows, counts


def conv3x3_dgrad_rows_nhwc(gy_nhwc, wd_crsk, rows, count_ptr, out=None):
    """gy (N,H,W,Cout), wd (Cin,3,3,Cout) flipped weights, rows: int32 device list (the dilation of gy's non-zero rows),
    count_ptr: device address of its length -> gx (N,H,W,Cin): the listed rows computed, all others zero.  `out`: only
    its listed rows are written."""
    L.need_device(gy_nhwc, wd_crsk, rows, out)
    N, H, W, Cout = gy_nhwc.shape
    Cin = wd_crsk.shape[0]
    if tuple(wd_crsk.shape) != (Cin, 3, 3, Cout) or not wd_crsk.is_contiguous():
        raise ValueError("wd must be a contiguous (Cin, 3, 3, Cout) tensor, got %r" % (tuple(wd_crsk.shape),))
    gy_nhwc = L.f32c(gy_nhwc)
    zero = out is None
    if zero:
        out = torch.empty((N, H, W, Cin), dtype=torch.float32, device=gy_nhwc.device)
    L.check(L.lib().jdet_conv3x3_dgrad_rows(L.ptr(gy_nhwc), L.ptr(wd_crsk), L.ptr(rows), count_ptr, N, H, W, Cin, Cout,
                                            int(zero), L.ptr(out), L.stream_ptr(gy_nhwc)), "jdet_conv3x3_dgrad_rows")
    return out


def _rows_backward(g, x, weight, need_x, need_w):
    """(grad_x, grad_w) of a plain 3x3 / stride 1 / pad 1 convolution from the non-zero rows of g (N, Cout, H, W)"""
    gn, xn = L.f32c(g.permute(0, 2, 3, 1)), L.f32c(x.permute(0, 2, 3, 1))
    _, rows, drows, counts = rows_nonzero(gn)
    gx = gw = None
    if need_w:
        gw = shared_wgrad(weight, xn, gn, rows=(rows, counts.data_ptr()))
    if need_x:
        gx = conv3x3_dgrad_rows_nhwc(gn, dgrad_weight(weight), drows, counts.data_ptr() + 4).permute(0, 3, 1, 2)
    return gx, gw


# Row-sparse FORWARD of a tower whose output only a positives-only loss reads (csrc/conv_rows.hip: jdet_rows_from_flags,
# jdet_conv3x3_rows_forward; profiles/conv_rows_fwd.md): the S2ANet head's ODM regression tower in training.  The layers
# are computed on the rows that feed a flagged position and are zero elsewhere; the backward is `_rows_backward`, so
# JDET_CONV_ROWS=0 switches the route off together with it, JDET_CONV_ROWS_FWD=0 the forward route alone (A/B).
ROWS_FWD = os.environ.get("JDET_CONV_ROWS_FWD", "1") == "1"


def rows_forward_supported(cin, cout):
    return bool(L.lib().jdet_conv3x3_rows_forward_supported(int(cin), int(cout)))


def rows_from_flags(flags, N, H, W):
    """flags: N*H*W bytes (uint8 / bool device tensor), non-zero = listed -> (rows, rows_dilated, rows_dilated2 (P,) int32,
    counts (3,) int32): the flagged positions, ascending, their 3x3 dilation inside each image and the dilation of that;
    list entries past their count are -1.  Everything stays on the device.  The four results are views of one fresh
    buffer (under graph capture: of the capturing graph's pool)."""
    L.need_device(flags)
    P = N * H * W
    if flags.numel() != P or flags.element_size() != 1 or not flags.is_contiguous():
        raise ValueError("flags must be %d contiguous bytes, got %r %s" % (P, tuple(flags.shape), flags.dtype))
    wsb = L.lib().jdet_rows_from_flags_workspace(N, H, W)
    buf = torch.empty((12 * P + 16 + wsb,), dtype=torch.uint8, device=flags.device)
    rows = [buf[4 * i * P:4 * (i + 1) * P].view(torch.int32) for i in range(3)]
    counts = buf[12 * P:12 * P + 12].view(torch.int32)
    ws = buf[12 * P + 16:]
    L.check(L.lib().jdet_rows_from_flags(L.ptr(flags), N, H, W, L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(rows[2]),
                                         L.ptr(counts), L.ptr(ws), wsb, L.stream_ptr(flags)), "jdet_rows_from_flags")
    return rows[0], rows[1], rows[2], counts


def conv3x3_rows_forward_nhwc(x_nhwc, w_krsc, bias, relu, rowmask, rows, count_ptr, out=None):
    """x (N,H,W,Cin), w (Cout,3,3,Cin), rows: int32 device list, count_ptr: device address of its length -> y
    (N,H,W,Cout): [relu](conv + bias) * rowmask on the listed rows, all others zero.  `out`: only its listed rows are
    written."""
    L.need_device(x_nhwc, w_krsc, bias, rowmask, rows, out)
    N, H, W, Cin = x_nhwc.shape
    Cout = w_krsc.shape[0]
    _check_shapes(N, H, W, Cin, w_krsc)
    x_nhwc, w_krsc = L.f32c(x_nhwc), L.f32c(w_krsc)
    zero = out is None
    if zero:
        out = torch.empty((N, H, W, Cout), dtype=torch.float32, device=x_nhwc.device)
    L.check(L.lib().jdet_conv3x3_rows_forward(
        L.ptr(x_nhwc), L.ptr(w_krsc), L.ptr(L.f32c(bias)) if bias is not None else None, int(bool(relu)),
        L.ptr(L.f32c(rowmask)) if rowmask is not None else None, L.ptr(rows), count_ptr, N, H, W, Cin, Cout, int(zero),
        L.ptr(out), L.stream_ptr(x_nhwc)), "jdet_conv3x3_rows_forward")
    return out


class _ConvBiasActRows(torch.autograd.Function):
    """y = [relu](conv3x3(x, w) + b) [* rowmask] on the listed rows, 0 on every other row.  Its backward is
    `_conv_backward` with `row_sparse` set: exact wherever the incoming gradient is zero outside the rows
    whose 3x3 neighbourhoods the list covers (a row that holds 0 has the ReLU mask [y > 0] = 0, as a masked row has)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, rowmask, rows, count_ptr):
        y = conv3x3_rows_forward_nhwc(L.f32c(x.permute(0, 2, 3, 1)), weight_krsc(weight), bias, relu, rowmask, rows,
                                      count_ptr).permute(0, 3, 1, 2)
        ctx.cfg = (bool(relu), bias is not None, [1, 1], [1, 1], [1, 1], 1, True, False, True)
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, g):
        return _conv_backward(ctx.saved_tensors, ctx.cfg, ctx.needs_input_grad, g) + (None,) * 4


def rows_tower_applicable(convs, x, positions=None):
    """can `rows_tower` run these layers on `x` (N, C, H, W) [or on a map of `positions` rows like it]?  At most two plain 3x3 / stride 1 / pad 1 nn.Conv2d layers
    with a trained bias (the one-pass bias backward supplies the ReLU mask), fp32 on the device, channel counts the
    gathered tile takes, both switches on."""
    if not (ROWS and ROWS_FWD and TRAIN and BIAS_ACT_BWD and 1 <= len(convs) <= 2):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    for conv in convs:
        if not (_plain_conv(conv) and _is_igemm_conv(conv) and conv.weight.dtype == torch.float32
                and conv.bias is not None and conv.bias.requires_grad and _bias_bwd_supported(conv.out_channels)
                and rows_forward_supported(conv.in_channels, conv.out_channels)
                and rows_supported(conv.in_channels, conv.out_channels)):
            return False
    P = x.shape[0] * x.shape[2] * x.shape[3] if positions is None else positions
    return _fits_32bit(P, max(c.in_channels for c in convs), max(c.out_channels for c in convs), 16)


def rows_tower(convs, x, flags, rowmask=None):
    """relu(conv(.)) [* rowmask] through one or two layers, computed only where the result feeds a 3x3 layer read at the
    flagged positions: the LAST layer on the 3x3 dilation of the flags, the one before it on the dilation of that; every
    other row of the result is zero.  flags: one byte per position of x (N*H*W), on the device."""
    N, _, H, W = x.shape
    lists = rows_from_flags(flags, N, H, W)
    counts = lists[3]
    n = len(convs)
    for i, conv in enumerate(convs):
        k = n - i                                   # dilations this layer's output is needed on
        x = _ConvBiasActRows.apply(x, conv.weight, conv.bias, True, rowmask, lists[k], counts.data_ptr() + 4 * k)
    return x


CONV1X1_GEMM = os.environ.get("JDET_CONV1X1_GEMM", "1") == "1"
# the library's data / weight gradients, called through this one name by both backwards below (tests wrap it to see which
# gradients a route left to the library: tests/test_gpu_conv_routes.py)
_convolution_backward = torch.ops.aten.convolution_backward


def _is_1x1(x, weight, stride, padding, groups):
    return (CONV1X1_GEMM and tuple(weight.shape[2:]) == (1, 1) and tuple(stride) == (1, 1) and tuple(padding) == (0, 0)
            and groups == 1 and x.is_cuda and x.dtype == torch.float32 and weight.shape[0] >= 64
            and x.is_contiguous(memory_format=torch.channels_last))


def _conv1x1_backward(g, x, weight, stride, padding, dilation, groups, need):
    """(grad_x, grad_w) of a stride-1 1x1 convolution of a channels-last map (`_is_1x1`)"""
    # the data gradient of a 1x1 convolution as gy . W (18 % faster than the library's over the ResNet / FPN
    # shapes), the weight gradient as gy^T . x only on small maps (its reduction runs over the positions)
    N, Ci, H, W = x.shape
    Co = weight.shape[0]
    g = g.contiguous(memory_format=torch.channels_last)
    gm = g.permute(0, 2, 3, 1).reshape(-1, Co)
    gx = gw1 = None
    if need[0]:
        gx = (gm @ weight.view(Co, Ci)).view(N, H, W, Ci).permute(0, 3, 1, 2)
        need[0] = False
    if need[1] and N * H * W <= 4096:
        gw1 = (gm.t() @ x.permute(0, 2, 3, 1).reshape(-1, Ci)).view(Co, Ci, 1, 1)
        need[1] = False
    _, gw, _ = _convolution_backward(g, x, weight, None, stride, padding, dilation, False,
                                     [0, 0], groups, need) if any(need) else (None, None, None)
    gw = gw1 if gw1 is not None else gw
    if gw is not None and gw.stride() != weight.stride() and gw.numel() == weight.numel():
        # (Cout, Cin, 1, 1) is one memory order under two stride spellings: the parameter's own keeps the
        # gradient layout contract (DDP's bucket views otherwise copy and warn)
        gw = gw.as_strided(weight.shape, weight.stride())
    return gx, gw


def _dgrad_route(g, weight, row_sparse, need_x, need_w):
    """who computes the data gradient of an igemm layer: "rows" = `_rows_backward` (the weight gradient with it),
    "bf16x3" = the split kernel on the flipped weights (the big layers), None = the library"""
    if not (g.is_cuda and g.dtype == torch.float32):
        return None
    P, cout, cin = g.shape[0] * g.shape[2] * g.shape[3], weight.shape[0], weight.shape[1]
    if row_sparse and ROWS and (need_x or need_w) and rows_supported(cin, cout) and _fits_32bit(P, cout, cin, 16):
        return "rows"
    if need_x and BF16X3_DGRAD and bf16x3_big(P, cout, cin):
        return "bf16x3"
    return None


def _conv_backward(saved, cfg, needs, g):
    """(grad_x, grad_w, grad_b) of y = [relu](conv(x, w) + b).  saved: (x, w, y or None); cfg: (relu, has_bias, stride,
    padding, dilation, groups, igemm, k1, row_sparse) as `_ConvBiasAct.forward` describes them; needs: which of the three
    are wanted.  Bias gradient and ReLU mask in one pass (`bias_act_backward`), then the own kernels where they apply,
    then the library's data / weight gradients for what is left."""
    x, weight, y = saved
    relu, has_bias, stride, padding, dilation, groups, igemm, k1, row_sparse = cfg
    gb = None
    if has_bias and needs[2]:
        g, gb = bias_act_backward(g, y, relu)
    elif relu:
        g = torch.ops.aten.threshold_backward(g, y, 0)
    need = [needs[0], needs[1], False]
    if k1:
        return _conv1x1_backward(g, x, weight, stride, padding, dilation, groups, need) + (gb,)
    route = _dgrad_route(g, weight, row_sparse, need[0], need[1]) if igemm else None
    if route == "rows":
        return _rows_backward(g, x, weight, need[0], need[1]) + (gb,)
    gx = gw = None
    if route == "bf16x3":
        gx = conv3x3_nhwc(L.f32c(g.permute(0, 2, 3, 1)), dgrad_weight(weight), bf16x3=True).permute(0, 3, 1, 2)
        need[0] = False
    if need[1] and igemm and WGRAD and wgrad_supported(weight.shape[1], weight.shape[0]):
        gw = shared_wgrad(weight, x.permute(0, 2, 3, 1), g.permute(0, 2, 3, 1))      # (None: added to an earlier use's)
        need[1] = False
    if any(need):
        lx, lw, _ = _convolution_backward(g, x, weight, None, stride, padding, dilation, False, [0, 0], groups, need)
        gx, gw = (lx if need[0] else gx), (lw if need[1] else gw)
    return gx, gw, gb


class _ConvBiasAct(torch.autograd.Function):
    """y = [relu](conv(x, w) + b).  Forward: the implicit-GEMM kernel (`igemm`: 3x3 / stride 1 / pad 1 only) or the
    library convolution; backward: `_conv_backward` (with BF16X3_DGRAD, for the big igemm shapes: grad_x by the bf16
    three-way-split kernel on the flipped weights).
    `row_sparse` (igemm layers): both gradients from the non-zero rows of the incoming gradient (`_rows_backward`)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, stride, padding, dilation, groups, igemm, rowmask=None, row_sparse=False):
        # rowmask (igemm + ReLU only): the finished rows are multiplied by a 0 / 1 mask per position (the gap rows of a
        # LevelPack).  It needs no backward of its own: a masked row of y is 0, so the ReLU mask [y > 0] of
        # bias_act_backward already zeroes the gradient there.
        k1 = _is_1x1(x, weight, stride, padding, groups)
        if igemm:
            y = conv3x3_nhwc(L.f32c(x.permute(0, 2, 3, 1)), weight_krsc(weight), bias, relu,
                             rowmask).permute(0, 3, 1, 2)
        elif k1 and weight.shape[1] >= 256 and x.shape[0] * x.shape[2] * x.shape[3] <= 32768:
            # stride-1 1x1 convolution of a channels-last map = GEMM on its (positions, channels) matrix view; the
            # forward wins from 256 input channels up (scripts/conv1x1_probe.py, profiles/r04_conv1x1_probe.txt)
            N, Ci, H, W = x.shape
            Co = weight.shape[0]
            xm = x.permute(0, 2, 3, 1).reshape(-1, Ci)
            ym = torch.addmm(bias, xm, weight.view(Co, Ci).t()) if bias is not None else xm @ weight.view(Co, Ci).t()
            if relu:
                ym = torch.relu_(ym)
            y = ym.view(N, H, W, Co).permute(0, 3, 1, 2)
        else:
            y = torch.ops.aten.convolution(x, weight, bias, stride, padding, dilation, False, [0, 0], groups)
            if relu:
                y = torch.relu_(y)
        ctx.cfg = (bool(relu), bias is not None, list(stride), list(padding), list(dilation), groups, bool(igemm), k1,
                   bool(row_sparse))
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, g):
        return _conv_backward(ctx.saved_tensors, ctx.cfg, ctx.needs_input_grad, g) + (None,) * 8


def conv3x3_bias_act(x, weight, bias=None, relu=False, rowmask=None, row_sparse=False):
    """(N, Cin, H, W) logical (channels_last memory is free) -> (N, Cout, H, W) channels_last; differentiable.
    rowmask: (N*H*W,) 0 / 1 floats multiplied into the finished rows (with relu=True and a bias when gradients flow:
    see _ConvBiasAct); row_sparse: the backward takes the rows path"""
    if needs_grad(x, weight, bias):
        return _ConvBiasAct.apply(x, weight, bias, relu, (1, 1), (1, 1), (1, 1), 1, True, rowmask, row_sparse)
    if rowmask is not None:
        return conv3x3_nhwc(L.f32c(x.permute(0, 2, 3, 1)), weight_krsc(weight), bias, relu, rowmask).permute(0, 3, 1, 2)
    return conv3x3(x, weight, bias, relu)


def _is_igemm_conv(conv):
    return ((conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups)
            == ((3, 3), (1, 1), (1, 1), (1, 1), 1))


def masked_conv_module(conv, x, rowmask, row_sparse=False):
    """`relu(conv(x)) * mask` in ONE kernel for a plain 3x3 / stride 1 / pad 1 nn.Conv2d with a bias where the fused
    kernel applies (the towers on a LevelPack); None = not applicable here, the caller multiplies."""
    plain = _plain_conv(conv)
    grad = needs_grad(x, conv.weight, conv.bias)
    if not (plain and _is_igemm_conv(conv) and preferred(x, conv.weight) and (TRAIN or not grad)):
        return None
    if grad and not (BIAS_ACT_BWD and conv.bias is not None and conv.bias.requires_grad
                     and _bias_bwd_supported(conv.out_channels)):
        return None          # (the ReLU mask of the one-pass bias backward is what zeroes the masked rows' gradient)
    return conv3x3_bias_act(x, conv.weight, conv.bias, True, rowmask, row_sparse)


def conv_module(conv, x, relu=False, row_sparse=False):
    """`[relu](conv(x))` for a plain nn.Conv2d (zeros padding).  3x3 / stride 1 / pad 1 layers take the fused kernel
    when `preferred()` says so; any layer WITH a bias that needs gradients goes through `_ConvBiasAct`, whose backward
    produces the bias gradient and the ReLU mask in one pass; everything else is the library call it always was."""
    plain = _plain_conv(conv)
    grad = needs_grad(x, conv.weight, conv.bias)
    # (prediction layers of 5 / 15 / 18 channels would run a 64-wide output tile three quarters empty: the library's
    # narrow-tile kernels keep their forward; their bias gradient still comes from the own column sum below)
    if (plain and _is_igemm_conv(conv) and conv.out_channels >= 32 and preferred(x, conv.weight)
            and (TRAIN or not grad)):
        return conv3x3_bias_act(x, conv.weight, conv.bias, relu, None, row_sparse)
    if (plain and grad and BIAS_ACT_BWD and conv.bias is not None and x.is_cuda and x.dtype == torch.float32
            and (_bias_bwd_supported(conv.out_channels) or (not relu and conv.out_channels <= 256))):
        return _ConvBiasAct.apply(x, conv.weight, conv.bias, relu, conv.stride, conv.padding, conv.dilation,
                                  conv.groups, False)
    y = conv(x)
    return torch.relu(y) if relu else y
