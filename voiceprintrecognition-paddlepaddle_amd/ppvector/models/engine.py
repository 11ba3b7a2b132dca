"""Host-side packing of model parameters into the C structs of include/vpmi.h, and the launch.

A packed engine owns contiguous device copies of the weights in the layout the kernels want
(conv weights [Cout][k*Cin] in the network dtype, BN folded to f32 scale/shift, the ASP context
columns split off, asp_bn / bn5 / bn6 folded into the last dense layer).  Packing is redone only
when a parameter's version counter or the package's raw-pointer weights epoch moves.
"""
import ctypes as C

import os

import torch

import ppvector
from ppvector import _native as N
from ppvector.models.utils import f32, pack_conv_weight, pack_hl32

_TORCH_DT = {'float32': torch.float32, 'float32x3': torch.float32, 'bfloat16': torch.bfloat16}


def _w1x1_t(conv):
    """Weight of a 1x1 Conv1D as f32 [in][out] (input-major): the SE and context-gate kernels read it that way."""
    return conv.weight.detach()[:, :, 0].float().t().contiguous()


def _versions(module):
    """Cache key of a packed engine: torch's version counters (in-place torch writes, load_state_dict) plus the epoch of
    raw-pointer writers (Adam step, train-mode BatchNorm statistics), which the counters do not see."""
    return (N.weights_epoch(),) + tuple(t._version for t in list(module.parameters()) + list(module.buffers()))


class _Engine:
    _ws_fn = _fwd_fn = None       # names of the backbone's vp_X_workspace_bytes / vp_X_fwd entry points (include/vpmi.h)

    def __init__(self, module, dtype_name):
        self.dtype_name = dtype_name
        self.tdtype = _TORCH_DT[dtype_name]
        self.dt = N.VP_F32X3 if dtype_name == 'float32x3' else N.dtype_id(self.tdtype)
        self.keep = []            # device tensors referenced by the C struct
        self.versions = _versions(module)
        self.device = next(module.parameters()).device
        self.ws = N.Workspace()
        self._slots = {}          # slot -> Workspace: one per concurrent launch sequence (forward_streams)
        self._streams = []

    def _p(self, t):
        if t is None:
            return None
        t = t.contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def conv_layer(self, L, conv, bn, kw_taps, w_packed, dil=1):
        """Fill a vp_tdnn_layer from packed weights [cout][kw_taps * cin]; conv gives the bias, bn (or None) the folded affine."""
        L.w = self._p(w_packed)
        self.split_weights(L, w_packed)
        L.bias = self._p(f32(conv.bias))
        if bn is not None:
            sc, sh = bn.folded()
            L.bn_scale, L.bn_shift = self._p(sc), self._p(sh)
        L.cin, L.cout, L.kw, L.dil = w_packed.shape[1] // kw_taps, w_packed.shape[0], kw_taps, dil

    def tdnn_layer(self, L, conv, bn, dil, w_override=None):
        """conv: _ConvParams (Conv1D, weight (cout, cin, kw)); bn: _BNParams or None."""
        w = w_override if w_override is not None else pack_conv_weight(conv.weight, self.tdtype)
        self.conv_layer(L, conv, bn, conv.weight.shape[2], w, dil)

    def split_weights(self, L, w):
        """'float32x3': the same [cout][K] weights as split bf16 planes, K zero-padded to a multiple of 32 (vp_tdnn_layer.w_hl) -- the conv
        kernels then split only the activations while staging, and ECAPA's fast path streams them by LDS-DMA."""
        if self.dtype_name == 'float32x3':
            kp = (w.shape[1] + 31) // 32 * 32
            L.w_hl = self._p(pack_hl32(torch.nn.functional.pad(w.float(), (0, kp - w.shape[1]))))

    def asp(self, A, asp):
        Cc = asp.channels
        w = asp.tdnn.conv.conv.weight.detach()[:, :, 0]                 # (att, 3C | C)
        wx = w[:, :Cc].to(self.tdtype).contiguous()
        self.tdnn_layer(A.tdnn, asp.tdnn.conv.conv, asp.tdnn.norm.norm, 1, w_override=wx)
        A.tdnn.cin, A.tdnn.kw = Cc, 1
        A.w_ctx = self._p(w[:, Cc:].float().contiguous()) if asp.global_context else None
        A.conv_w = self._p(pack_conv_weight(asp.conv.conv.weight, self.tdtype))
        A.conv_b = self._p(f32(asp.conv.conv.bias))
        A.C, A.att = Cc, asp.attention_channels

    def workspace(self, nbytes, device, slot=0):
        """Grow-only scratch of launch sequence `slot`: sequences that run concurrently on different streams must not share one."""
        if slot == 0:
            return self.ws.get(nbytes, device)
        w = self._slots.get(slot)
        if w is None:
            w = self._slots[slot] = N.Workspace()
        return w.get(nbytes, device)

    def forward_streams(self, x, n_streams, producer=None):
        """The same forward as `forward`, the batch cut into `n_streams` contiguous shards that run as independent launch
        sequences on side streams (own workspace each).  Utterances are independent in eval mode, so results are bit-identical;
        the point is packing: a 512 -> 512 layer of a 256-utterance batch is 596 tiles on 256 CUs (2.33 rounds) and the
        HBM-bound kernels between the GEMMs leave the matrix cores idle -- with several sequences in flight the idle CUs of one
        take the tiles of another (measured on MI355X, ECAPA B = 256: 1.51 ms -> 1.43 (2 streams) -> 1.36 (4)).
        `producer(x_shard) -> features` (optional) runs at the head of each shard's sequence, e.g. the featurizer over a shard of
        waveforms, so that the front end of one shard overlaps the backbone of another."""
        B = x.shape[0]
        S = max(1, min(int(n_streams), B))
        while len(self._streams) < S:
            self._streams.append(torch.cuda.Stream(device=x.device))
        cur = torch.cuda.current_stream(x.device)
        emb = torch.empty((B, self.W.embd_dim), dtype=torch.float32, device=x.device)
        bounds = [(B * i) // S for i in range(S + 1)]
        for i in range(S):
            st = self._streams[i]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                xs = x[bounds[i]:bounds[i + 1]]
                if producer is not None:
                    xs = producer(xs)
                self._launch(self.feats_in(xs), emb[bounds[i]:bounds[i + 1]], slot=i + 1)
        for i in range(S):
            cur.wait_stream(self._streams[i])      # everything allocated above is reused only behind this join
        return emb

    def _launch(self, xin, emb, slot=0):
        B, T, F = xin.shape
        lib, ctx = N.lib(), N.ctx(xin.device)
        nws = getattr(lib, self._ws_fn)(C.byref(self.W), B, T)
        ws = self.workspace(nws, xin.device, slot)
        N.check(getattr(lib, self._fwd_fn)(ctx, C.byref(self.W), xin.data_ptr(), B, T, emb.data_ptr(), ws.data_ptr(),
                                           ws.numel(), N.stream_ptr()), ctx)

    def forward(self, x):
        xin = self.feats_in(x)
        emb = torch.empty((xin.shape[0], self.W.embd_dim), dtype=torch.float32, device=xin.device)
        self._launch(xin, emb)
        return emb

    def feats_in(self, x):
        """(B,T,F) f32 (API contract) -> tensor in the network dtype (no copy on the f32 path)."""
        if not x.is_cuda:
            raise N.VpmiError('model input must be a GPU tensor: the engine has no CPU fallback')
        if self.tdtype == torch.float32:
            return x.contiguous().float()
        twin = getattr(x, '_vp_bf16', None)
        if twin is not None and twin.shape == x.shape:
            return twin
        if x.dtype == torch.bfloat16:
            return x.contiguous()
        x = x.contiguous().float()
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        ctx = N.ctx(x.device)
        N.check(N.lib().vp_cast_f32_bf16(ctx, x.data_ptr(), y.data_ptr(), x.numel(), N.stream_ptr()), ctx)
        return y


class EcapaEngine(_Engine):
    _ws_fn, _fwd_fn = 'vp_ecapa_workspace_bytes', 'vp_ecapa_fwd'

    def __init__(self, m, dtype_name):
        super().__init__(m, dtype_name)
        W = N.EcapaWeights()
        W.dtype, W.feat_dim, W.embd_dim = self.dt, m.input_size, m.embd_dim
        W.n_blocks, W.res2_scale, W.se_ch = len(m.blocks) - 1, m.res2net_scale, m.se_channels
        b0 = m.blocks[0]
        self.tdnn_layer(W.block0, b0.conv.conv, b0.norm.norm, b0.conv.dilation)
        for i, blk in enumerate(list(m.blocks)[1:]):
            if blk.shortcut is not None:
                raise NotImplementedError('SERes2NetBlock with in_channels != out_channels (shortcut conv) is not built')
            S = W.blk[i]
            self.tdnn_layer(S.tdnn1, blk.tdnn1.conv.conv, blk.tdnn1.norm.norm, 1)
            for j, rb in enumerate(blk.res2net_block.blocks):
                self.tdnn_layer(S.res2[j], rb.conv.conv, rb.norm.norm, rb.conv.dilation)
            self.tdnn_layer(S.tdnn2, blk.tdnn2.conv.conv, blk.tdnn2.norm.norm, 1)
            S.se_w1 = self._p(_w1x1_t(blk.se_block.conv1.conv))     # [C][se_ch]
            S.se_b1 = self._p(f32(blk.se_block.conv1.conv.bias))
            S.se_w2 = self._p(_w1x1_t(blk.se_block.conv2.conv))     # [se_ch][C]
            S.se_b2 = self._p(f32(blk.se_block.conv2.conv.bias))
        self.tdnn_layer(W.mfa, m.mfa.conv.conv, m.mfa.norm.norm, m.mfa.conv.dilation)
        self.asp(W.asp, m.asp)
        # asp_bn folded into fc: fc(bn(p)) = (W*scale) p + (b + W shift)
        sc, sh = m.asp_bn.norm.folded()
        fw = m.fc.conv.weight.detach()[:, :, 0].float()
        W.fc_w = self._p(fw * sc[None, :])
        W.fc_b = self._p(m.fc.conv.bias.detach().float() + fw @ sh)
        self.W = W

    def x3_fast_path(self, B, T):
        """True when forward() of a (B, T) batch takes the split-plane fast path of the 'float32x3' engine (csrc/ecapa.hip:
        ecapa_hl_ok), False on the generic split-precision path and on the other engines.  Host only: needs no GPU."""
        return bool(N.lib().vp_ecapa_x3_fast_path(C.byref(self.W), int(B), int(T)))


class TdnnEngine(_Engine):
    _ws_fn, _fwd_fn = 'vp_tdnn_workspace_bytes', 'vp_tdnn_fwd'

    def __init__(self, m, dtype_name):
        super().__init__(m, dtype_name)
        W = N.TdnnWeights()
        W.dtype, W.feat_dim, W.embd_dim, W.channels = self.dt, m.input_size, m.embd_dim, m.channels
        convs = [m.td_layer1, m.td_layer2, m.td_layer3, m.td_layer4, m.td_layer5]
        bns = [m.bn1, m.bn2, m.bn3, m.bn4, None]
        for i, (cv, bn, d) in enumerate(zip(convs, bns, (1, 2, 3, 1, 1))):
            self.tdnn_layer(W.td[i], cv, bn, d)
        self.asp(W.asp, m.pooling)
        # bn5 and bn6 folded around the Linear (Paddle weight [in, out])
        s5, h5 = m.bn5.norm.folded()
        s6, h6 = m.bn6.norm.folded()
        lw = m.linear.weight.detach().float().t()                     # [out, in]
        lb = m.linear.bias.detach().float()
        W.lin_w = self._p(lw * s5[None, :] * s6[:, None])
        W.lin_b = self._p((lb + lw @ h5) * s6 + h6)
        self.W = W


class CamppEngine(_Engine):
    """Packs a CAMPPlus module into vp_campplus_weights (include/vpmi.h)."""
    _ws_fn, _fwd_fn = 'vp_campplus_workspace_bytes', 'vp_campplus_fwd'

    def conv2d(self, L, conv, bn):
        w = conv.weight.detach()                                  # (Cout, Cin, kF, kT)
        kf, kt = w.shape[2], w.shape[3]
        wp = w.permute(0, 3, 2, 1).reshape(w.shape[0], kt * kf * w.shape[1]).to(self.tdtype).contiguous()
        self.conv_layer(L, conv, bn, kt * kf, wp)

    def __init__(self, m, dtype_name):
        super().__init__(m, dtype_name)
        W = N.CamppWeights()
        head, xv = m.head, m.xvector
        W.dtype, W.feat_dim, W.embd_dim, W.m_channels = self.dt, m.input_size, m.embd_dim, head.conv1.weight.shape[0]
        W.init_channels, W.growth, W.bn_channels, W.seg_len = m.init_channels, m.growth_rate, m.bn_size * m.growth_rate, 100
        W.n_blocks = len(m.block_cfg)
        for i, (nl, _, _) in enumerate(m.block_cfg):
            W.block_layers[i] = nl
        w1 = head.conv1.weight.detach()[:, 0]                       # (32, kF, kT)
        W.fcm1_w = self._p(w1.permute(0, 2, 1).reshape(w1.shape[0], 9).float())
        W.fcm1_b = self._p(f32(head.conv1.bias))
        sc, sh = head.bn1.folded()
        W.fcm1_scale, W.fcm1_shift = self._p(sc), self._p(sh)
        blocks = list(head.layer1) + list(head.layer2)
        for i, rb in enumerate(blocks):
            R = W.res[i]
            self.conv2d(R.conv1, rb.conv1, rb.bn1)
            self.conv2d(R.conv2, rb.conv2, rb.bn2)
            R.stride = rb.stride
            R.has_shortcut = int(len(rb.shortcut) > 0)
            if R.has_shortcut:
                self.conv2d(R.shortcut, rb.shortcut[0], rb.shortcut[1])
        self.conv2d(W.fcm_conv2, head.conv2, head.bn2)
        # TDNN k5 s2: reference input channel = c * F' + f (reshape of (B, C, F', T)); ours = f * 32 + c
        tw = xv.tdnn.linear.weight.detach()                         # (init, 32*F', 5)
        C32 = W.m_channels
        Fq = tw.shape[1] // C32
        twp = tw.reshape(tw.shape[0], C32, Fq, tw.shape[2]).permute(0, 3, 2, 1).reshape(tw.shape[0], -1)
        self.conv_layer(W.tdnn, xv.tdnn.linear, xv.tdnn.nonlinear.batchnorm, tw.shape[2], twp.to(self.tdtype).contiguous())
        li = 0
        for bi, (nl, k, d) in enumerate(m.block_cfg, start=1):
            blk = getattr(xv, f'block{bi}')
            for l in range(1, nl + 1):
                lay = getattr(blk, f'tdnnd{l}')
                L = W.layers[li]
                s1, h1 = lay.nonlinear1.batchnorm.folded()
                L.bn1_scale, L.bn1_shift = self._p(s1), self._p(h1)
                self.conv_layer(L.linear1, lay.linear1, lay.nonlinear2.batchnorm, 1,
                                lay.linear1.weight.detach()[:, :, 0].to(self.tdtype).contiguous())
                cl = lay.cam_layer
                self.conv_layer(L.local, cl.linear_local, None, k, pack_conv_weight(cl.linear_local.weight, self.tdtype), d)
                L.ctx_w1 = self._p(_w1x1_t(cl.linear1))
                L.ctx_b1 = self._p(f32(cl.linear1.bias))
                L.ctx_w2 = self._p(_w1x1_t(cl.linear2))
                L.ctx_b2 = self._p(f32(cl.linear2.bias))
                li += 1
            tr = getattr(xv, f'transit{bi}')
            Tr = W.transit[bi - 1]
            ts, th = tr.nonlinear.batchnorm.folded()
            Tr.bn_scale, Tr.bn_shift = self._p(ts), self._p(th)
            self.conv_layer(Tr.linear, tr.linear, None, 1, tr.linear.weight.detach()[:, :, 0].to(self.tdtype).contiguous())
        os_, oh = xv.out_nonlinear.batchnorm.folded()
        W.out_bn_scale, W.out_bn_shift = self._p(os_), self._p(oh)
        ds, dh = xv.dense.nonlinear.batchnorm.folded()
        dw = xv.dense.linear.weight.detach()[:, :, 0].float()
        W.dense_w = self._p(dw * ds[:, None])
        W.dense_b = self._p(xv.dense.linear.bias.detach().float() * ds + dh)
        self.W = W


def _pack_permuted_asp_head(eng, W, m, C4, Fq):
    """ASP -> bn2 -> Linear -> bn3 over the (B, C4*Fq, T') reshape of a 2-D backbone's last map (ResNetSE, Res2Net).  The reference's
    channel index after the reshape is c * Fq + f; the engine keeps (B, T', F', C): f * C4 + c, so the ASP and Linear weights are
    permuted here, and bn2 / bn3 are folded into the Linear."""
    Cc = C4 * Fq

    def perm_cols(w):                                               # (..., k*Cc) columns c*Fq+f -> f*C4+c per Cc group
        lead = w.shape[:-1]
        k = w.shape[-1] // Cc
        return w.reshape(*lead, k, C4, Fq).transpose(-1, -2).reshape(*lead, k * Cc)

    asp, A = m.pooling, W.asp
    w = perm_cols(asp.tdnn.conv.conv.weight.detach()[:, :, 0])      # (att, 3 Cc)
    eng.tdnn_layer(A.tdnn, asp.tdnn.conv.conv, asp.tdnn.norm.norm, 1, w_override=w[:, :Cc].to(eng.tdtype).contiguous())
    A.tdnn.cin, A.tdnn.kw = Cc, 1
    A.w_ctx = eng._p(w[:, Cc:].float().contiguous())
    cw = asp.conv.conv.weight.detach()[:, :, 0]                     # (Cc, att): permute output rows
    A.conv_w = eng._p(cw.reshape(C4, Fq, -1).transpose(0, 1).reshape(Cc, -1).to(eng.tdtype).contiguous())
    A.conv_b = eng._p(asp.conv.conv.bias.detach().float().reshape(C4, Fq).t().reshape(-1).contiguous())
    A.C, A.att = Cc, asp.attention_channels
    # bn3(linear(bn2(p))): fold both affines into one dense layer over the permuted pooled vector
    s2, h2 = m.bn2.norm.folded()
    s3, h3 = m.bn3.norm.folded()
    lw = m.linear.weight.detach().float()                           # [2Cc, embd] (Paddle layout)
    wt = (lw * s2[:, None]).t() * s3[:, None]                       # (embd, 2Cc)
    W.lin_w = eng._p(perm_cols(wt).contiguous())
    W.lin_b = eng._p(((h2 @ lw) + m.linear.bias.detach().float()) * s3 + h3)


class ResNetSEEngine(CamppEngine):
    """Packs a ResNetSE module into vp_resnetse_weights (include/vpmi.h)."""
    _ws_fn, _fwd_fn = 'vp_resnetse_workspace_bytes', 'vp_resnetse_fwd'

    def __init__(self, m, dtype_name):
        _Engine.__init__(self, m, dtype_name)
        W = N.ResnetSeWeights()
        W.dtype, W.feat_dim, W.embd_dim, W.c1_channels = self.dt, m.input_size, m.embd_dim, m.conv1.weight.shape[0]
        if m.input_size % 8:
            raise NotImplementedError('ResNetSE on the HIP engine needs input_size % 8 == 0 (the reference sizes its '
                                      'pooling for input_size // 8 bins)')
        w1 = m.conv1.weight.detach()[:, 0]                          # (32, kF, kT)
        W.c1_w = self._p(w1.permute(0, 2, 1).reshape(w1.shape[0], 9).float())
        W.c1_b = self._p(f32(m.conv1.bias))
        sc, sh = m.bn1.folded()
        W.c1_scale, W.c1_shift = self._p(sc), self._p(sh)
        blocks = [b for l in (m.layer1, m.layer2, m.layer3, m.layer4) for b in l]
        if len(blocks) > N.VP_MAX_RSE_BLOCKS:
            raise NotImplementedError(f'more than {N.VP_MAX_RSE_BLOCKS} bottleneck blocks')
        W.n_blocks = len(blocks)
        for i, b in enumerate(blocks):
            R = W.blk[i]
            self.conv2d(R.conv1, b.conv1, b.bn1)
            self.conv2d(R.conv2, b.conv2, b.bn2)
            self.conv2d(R.conv3, b.conv3, b.bn3)
            R.se_w1, R.se_b1 = self._p(f32(b.se.fc[0].weight)), self._p(f32(b.se.fc[0].bias))
            R.se_w2, R.se_b2 = self._p(f32(b.se.fc[2].weight)), self._p(f32(b.se.fc[2].bias))
            st = b.stride[0] if isinstance(b.stride, (tuple, list)) else b.stride
            R.stride, R.has_down = st, int(b.downsample is not None)
            if R.has_down:
                self.conv2d(R.down, b.downsample[0], b.downsample[1])
        _pack_permuted_asp_head(self, W, m, blocks[-1].conv3.weight.shape[0], m.input_size // 8)
        self.W = W


def _ceil8(v):
    return (v + 7) // 8 * 8


def _chunk_map(width, wp, nchunk):
    """old channel i*width + j  ->  padded channel i*wp + j  (Res2 chunks padded to a multiple of 8 channels)."""
    return torch.cat([torch.arange(width) + i * wp for i in range(nchunk)])


class Eres2netEngine(CamppEngine):
    """Packs an ERes2Net / ERes2NetV2 module into vp_eres2net_weights (include/vpmi.h).  Chunk widths that are not multiples
    of 8 (V2: 13 / 26 / 52 / 104) are zero-padded: padded channels carry zero weights, zero bias and a zero BN affine, so they
    stay exactly 0 through Hardtanh / SiLU / tanh and the AFF combine, and meet zero weight columns downstream."""
    _ws_fn, _fwd_fn = 'vp_eres2net_workspace_bytes', 'vp_eres2net_fwd'

    def conv2d_pad(self, L, conv, bn, in_map=None, cin_p=None, out_map=None, cout_p=None):
        w = conv.weight.detach().float()                            # (Cout, Cin, kF, kT)
        cout, cin, kf, kt = w.shape
        cin_p, cout_p = cin_p or cin, cout_p or cout
        in_map = torch.arange(cin) if in_map is None else in_map
        out_map = torch.arange(cout) if out_map is None else out_map
        wpad = torch.zeros((cout_p, cin_p, kf, kt), dtype=torch.float32, device=w.device)
        wpad[out_map.to(w.device)[:, None], in_map.to(w.device)[None, :]] = w
        packed = wpad.permute(0, 3, 2, 1).reshape(cout_p, kt * kf * cin_p).to(self.tdtype).contiguous()
        L.w = self._p(packed)
        self.split_weights(L, packed)
        bias = torch.zeros(cout_p, dtype=torch.float32, device=w.device)
        bias[out_map.to(w.device)] = conv.bias.detach().float()
        L.bias = self._p(bias)
        if bn is not None:
            sc, sh = bn.folded()
            scp = torch.zeros(cout_p, dtype=torch.float32, device=w.device)
            shp = torch.zeros(cout_p, dtype=torch.float32, device=w.device)
            scp[out_map.to(w.device)] = sc
            shp[out_map.to(w.device)] = sh
            L.bn_scale, L.bn_shift = self._p(scp), self._p(shp)
        L.cin, L.cout, L.kw, L.dil = cin_p, cout_p, kt * kf, 1

    def aff(self, A, m, width=None, wp=None):
        la = m.local_att
        if width is None:                                           # stage-level AFF: channel counts are multiples of 64
            self.conv2d_pad(A.c1, la[0], la[1])
            self.conv2d_pad(A.c2, la[3], la[4])
            return
        inter = la[0].weight.shape[0]
        ip = _ceil8(inter)
        self.conv2d_pad(A.c1, la[0], la[1], in_map=_chunk_map(width, wp, 2), cin_p=2 * wp, cout_p=ip)
        self.conv2d_pad(A.c2, la[3], la[4], cin_p=ip, cout_p=wp)

    def __init__(self, m, dtype_name):
        _Engine.__init__(self, m, dtype_name)
        W = N.Eres2netWeights()
        W.dtype, W.feat_dim, W.embd_dim, W.m_channels = self.dt, m.input_size, m.embd_dim, m.m_channels
        if m.input_size % 8 or m.m_channels % 8 or m.m_channels > 64:
            raise NotImplementedError('ERes2Net on the HIP engine needs input_size % 8 == 0 and m_channels in {8..64, % 8}')
        w1 = m.conv1.weight.detach()[:, 0]                          # (m, kF, kT)
        W.c1_w = self._p(w1.permute(0, 2, 1).reshape(w1.shape[0], 9).float())
        W.c1_b = self._p(f32(m.conv1.bias))
        sc, sh = m.bn1.folded()
        W.c1_scale, W.c1_shift = self._p(sc), self._p(sh)
        bi = 0
        for s, layer in enumerate((m.layer1, m.layer2, m.layer3, m.layer4)):
            W.stage_blocks[s] = len(layer)
            for b in layer:
                if bi >= N.VP_MAX_ERE_BLOCKS or b.scale > N.VP_MAX_ERE_SCALE:
                    raise NotImplementedError(f'more than {N.VP_MAX_ERE_BLOCKS} blocks or scale > {N.VP_MAX_ERE_SCALE}')
                R = W.blk[bi]
                wd, wp = b.width, _ceil8(b.width)
                cmap = _chunk_map(wd, wp, b.scale)
                self.conv2d_pad(R.conv1, b.conv1, b.bn1, out_map=cmap, cout_p=wp * b.scale)
                for i in range(b.scale):
                    self.conv2d_pad(R.convs[i], b.convs[i], b.bns[i], cin_p=wp, cout_p=wp)
                self.conv2d_pad(R.conv3, b.conv3, b.bn3, in_map=cmap, cin_p=wp * b.scale)
                R.has_shortcut = int(len(b.shortcut) > 0)
                if R.has_shortcut:
                    self.conv2d_pad(R.shortcut, b.shortcut[0], b.shortcut[1])
                R.use_aff = int(b.use_aff)
                if b.use_aff:
                    for i in range(b.scale - 1):
                        self.aff(R.fuse[i], b.fuse_models[i], wd, wp)
                R.stride, R.width, R.scale = b.stride, wp, b.scale
                bi += 1
        W.n_blocks = bi
        if getattr(m, 'v2', False):                                 # ERes2NetV2: one fusion, kept in slot 2
            W.first_fuse = 2
            self.conv2d_pad(W.down[2], m.layer3_ds, None)
            self.aff(W.fuse[2], m.fuse34)
            C4 = m.layer3_ds.weight.shape[0]
        else:
            W.first_fuse = 0
            for k, (dn, fm) in enumerate(((m.layer1_downsample, m.fuse_mode12), (m.layer2_downsample, m.fuse_mode123),
                                          (m.layer3_downsample, m.fuse_mode1234))):
                self.conv2d_pad(W.down[k], dn, None)
                self.aff(W.fuse[k], fm)
            C4 = m.layer3_downsample.weight.shape[0]
        # TSTP vector: reference index stat*(C*F8) + c*F8 + f  ->  engine stat*(F8*C) + f*C + c
        F8 = m.input_size // 8
        lw = m.seg_1.weight.detach().float()                        # [2*C4*F8, embd] (Paddle layout)
        if lw.shape[0] != 2 * C4 * F8:
            raise NotImplementedError(f'seg_1 expects {lw.shape[0]} statistics, the backbone produces {2 * C4 * F8}')
        wt = lw.t().reshape(-1, 2, C4, F8).transpose(2, 3).reshape(-1, 2 * C4 * F8)
        W.seg_w = self._p(wt.contiguous())
        W.seg_b = self._p(f32(m.seg_1.bias))
        self.W = W


class Res2NetEngine(Eres2netEngine):
    """Packs a Res2Net module into vp_res2net_weights (include/vpmi.h).  The concat of a Bottle2neck is kept as [last chunk | sp_0 |
    ... | sp_{nums-1}]: conv1's output channels and conv3's input channels are permuted to that order (the pass-through chunk then
    comes out of conv1's epilogue, csrc/res2net.hip).  Chunk widths that are not multiples of 8 are zero-padded as in ERes2Net."""
    _ws_fn, _fwd_fn = 'vp_res2net_workspace_bytes', 'vp_res2net_fwd'

    def __init__(self, m, dtype_name):
        _Engine.__init__(self, m, dtype_name)
        W = N.Res2netWeights()
        W.dtype, W.feat_dim, W.embd_dim, W.m_channels = self.dt, m.input_size, m.embd_dim, m.m_channels
        if m.m_channels % 8 or m.m_channels > 256:
            raise NotImplementedError('Res2Net on the HIP engine needs m_channels a multiple of 8, at most 256')
        w1 = m.conv1.weight.detach()[:, 0]                          # (m, kF, kT)
        W.c1_w = self._p(w1.permute(0, 2, 1).reshape(w1.shape[0], 49).float())
        W.c1_b = self._p(f32(m.conv1.bias))
        sc, sh = m.bn1.folded()
        W.c1_scale, W.c1_shift = self._p(sc), self._p(sh)
        blocks = [b for l in (m.layer1, m.layer2, m.layer3, m.layer4) for b in l]
        if len(blocks) > N.VP_MAX_R2N_BLOCKS or m.scale > N.VP_MAX_R2N_SCALE:
            raise NotImplementedError(f'more than {N.VP_MAX_R2N_BLOCKS} blocks or scale > {N.VP_MAX_R2N_SCALE}')
        W.n_blocks = len(blocks)
        for i, b in enumerate(blocks):
            R = W.blk[i]
            S, wd = b.scale, b.width
            wp = _ceil8(wd)
            slots = [k + 1 for k in range(S - 1)] + [0] if S > 1 else [0]     # reference chunk k -> engine slot
            cmap = torch.cat([torch.arange(wd) + slots[k] * wp for k in range(S)])
            self.conv2d_pad(R.conv1, b.conv1, b.bn1, out_map=cmap, cout_p=wp * S)
            for j in range(b.nums):
                self.conv2d_pad(R.convs[j], b.convs[j], b.bns[j], cin_p=wp, cout_p=wp)
            self.conv2d_pad(R.conv3, b.conv3, b.bn3, in_map=cmap, cin_p=wp * S)
            R.has_down = int(b.downsample is not None)
            if R.has_down:
                self.conv2d_pad(R.down, b.downsample[0], b.downsample[1])
            R.stride, R.stage, R.width, R.scale = b.stride, int(b.stype == 'stage'), wp, S
        from ppvector.models.res2net import feature_bins
        _pack_permuted_asp_head(self, W, m, blocks[-1].conv3.weight.shape[0], feature_bins(m.input_size))
        self.W = W


def _graph_forward(eng, x):
    """Replay the engine's launch sequence for this (shape, dtype) from a captured HIP graph.  Static input / output buffers
    belong to the graph; the result is copied out so the caller owns it."""
    xin = eng.feats_in(x)
    key = (tuple(xin.shape), xin.dtype)
    graphs = eng.__dict__.setdefault('_graphs', {})
    ent = graphs.get(key)
    if ent is None:
        static_in = xin.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up outside capture: workspace growth, attribute calls
            eng.forward(static_in)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            static_out = eng.forward(static_in)
        ent = graphs[key] = (g, static_in, static_out)
    g, static_in, static_out = ent
    static_in.copy_(xin)
    g.replay()
    return static_out.clone()


class EngineMixin:
    """forward() of a backbone: eval-mode fused forward on the HIP engine."""
    _engine_cls = None

    def engine(self, dtype_name=None):
        dtype_name = dtype_name or ppvector.get_compute_dtype()
        cache = self.__dict__.setdefault('_engines', {})
        e = cache.get(dtype_name)
        if e is None or e.versions != _versions(self) or e.device != next(self.parameters()).device:
            if dtype_name == 'bfloat16':
                import warnings
                err = getattr(self, '_bf16_trained_score_err', None)
                warnings.warn(f'{type(self).__name__}: the bf16 engine is outside the 1e-4 reference tolerance: at trained weights its all-pairs '
                              f'cosine scores differ from the f32 reference by {err if err else "2e-3 .. 4e-2"} (measured on MI355X, '
                              "tests/test_gpu_models.py::test_score_parity_at_trained_weights).  " +
                              ("The 'float32' engine (the default) meets it" if getattr(self, '_x3_trained_score_err', None) else
                               "The 'float32' engine (the default) and the split-precision 'float32x3' engine meet it"),
                              RuntimeWarning, stacklevel=2)
            elif dtype_name == 'float32x3' and getattr(self, '_x3_trained_score_err', None):
                import warnings
                warnings.warn(f"{type(self).__name__}: the split-precision 'float32x3' engine is outside the 1e-4 reference tolerance on this "
                              f'backbone: at trained weights its all-pairs cosine scores differ from the f32 reference by '
                              f'{self._x3_trained_score_err} (measured on MI355X).  The \'float32\' engine (the default) meets it',
                              RuntimeWarning, stacklevel=2)
            with torch.no_grad():
                e = self._engine_cls(self, dtype_name)
            cache[dtype_name] = e
        return e

    def forward(self, x, lengths=None):
        if lengths is not None:
            raise NotImplementedError('lengths= is never passed by the reference entry points (trainer.py:210); '
                                      'the masked branches are not built')
        if self.training:
            fwd = getattr(self, '_train_forward', None)
            if fwd is None:
                raise NotImplementedError(f'training-mode forward/backward on the HIP engine is not built for {type(self).__name__} '
                                          '(TDNN, EcapaTdnn, CAMPPlus, ResNetSE, ERes2Net, ERes2NetV2 and Res2Net are: DESIGN.md section 7a); '
                                          'call .eval() for embedding extraction')
            N.bump_weights_epoch()                 # the train-mode forward rewrites the BatchNorm running statistics in place
            return fwd(x)
        with torch.no_grad():
            eng = self.engine()
            if ppvector.get_graph_mode():
                return _graph_forward(eng, x)
            ns = ppvector.get_forward_streams()
            if ns > 1 and x.shape[0] >= 32 * ns:
                return eng.forward_streams(x, ns)
            return eng.forward(x)
