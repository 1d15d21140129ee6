"""RRDBNet, the Residual-in-Residual Dense Block generator of ESRGAN / Real-ESRGAN / BSRGAN, and its meta-attention form,
on the HIP path.

The parameter names are BasicSR's (conv_first, body.{i}.rdb{1,2,3}.conv{1..5}, conv_body, conv_up1, conv_up2, conv_hr,
conv_last; OIHW), so a public generator checkpoint (RRDB_PSNR_x4, RealESRGAN_x4plus) loads with load_state_dict as it is.

  f   = conv_first(x)
  f   = f + conv_body(body(f))                       body: num_blocks RRDBs
  f   = lrelu(conv_up1(nearest x2(f)));  f = lrelu(conv_up2(nearest x2(f)))
  out = conv_last(lrelu(conv_hr(f)))                 lrelu = LeakyReLU(0.2)
  RDB(x)  = conv5(cat(x, x_1 .. x_4)) * 0.2 + x,  x_j = lrelu(conv_j(cat(x, x_1 .. x_{j-1})))
  RRDB(x) = rdb3(rdb2(rdb1(x))) * 0.2 + x;        QRRDB(x, m) = (rdb3(rdb2(rdb1(x))) * m) * 0.2 + x

Routing: every RDB is one ops.dense_block node on the dense-block kernels (csrc/dense.hip) working in place in a 192-channel
stack, the RRDB skip ops.dense_skip from one stack into the next; conv_first / conv_last the RGB-end kernels; conv_body the
64 -> 64 conv with the long skip fused; the two up-sampling convs and conv_hr ops.conv_chain with the LeakyReLU epilogue behind
ops.nearest_up.  The nn.Conv2d children are parameter holders only.
"""
import torch
from torch import nn

from . import ops
from .architectures import ParaCALayer, _check_rgb, meta_gates
from .handlers import BaseModel, L1Loss, QModel

SLOPE, RES_SCALE = 0.2, 0.2  # (ops.conv_chain's LeakyReLU epilogue, act code 2, is LeakyReLU(0.2) too)


def _init_dense(convs, scale=0.1):
    """BasicSR's default_init_weights(scale=0.1): Kaiming-normal (fan_in, a = 0) x scale, zero bias"""
    for m in convs:
        nn.init.kaiming_normal_(m.weight, a=0, mode='fan_in')
        with torch.no_grad():
            m.weight.mul_(scale)
            m.bias.zero_()


class ResidualDenseBlock(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        for j in range(1, 5):
            setattr(self, 'conv%d' % j, nn.Conv2d(num_feat + (j - 1) * num_grow_ch, num_grow_ch, 3, 1, 1))
        self.conv5 = nn.Conv2d(num_feat + 4 * num_grow_ch, num_feat, 3, 1, 1)
        _init_dense(self.convs())

    def convs(self):
        return [getattr(self, 'conv%d' % j) for j in range(1, 6)]

    def forward(self, x):
        return ops.dense_block(x, [(m.weight, m.bias) for m in self.convs()], slope=SLOPE, alpha=RES_SCALE)


class RRDB(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        self.rdb1 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb2 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb3 = ResidualDenseBlock(num_feat, num_grow_ch)

    def forward(self, x, gate=None):
        """gate: (B, 64) meta-attention gate m of this block (QRRDB), or None"""
        t = self.rdb3(self.rdb2(self.rdb1(x)))
        if gate is None:
            g = _const_gate(x.shape[0], x.device)
        else:
            g = gate.reshape(x.shape[0], 64) * RES_SCALE
        return ops.dense_skip(t, g, x)


_const_gates = {}


def _const_gate(B, device):
    key = (B, device.index)
    g = _const_gates.get(key)
    if g is None:
        g = _const_gates[key] = torch.full((B, 64), RES_SCALE, device=device)
    return g


class QRRDB(RRDB):
    """an RRDB that owns the ParaCALayer whose gate scales its residual branch"""

    def __init__(self, num_feat=64, num_grow_ch=32, input_para=1, q_layer_nonlinearity=False):
        super().__init__(num_feat, num_grow_ch)
        self.attention_layer = ParaCALayer(num_feat, input_para, nonlinearity=q_layer_nonlinearity)


def _refuse(scale, num_features, num_grow_ch, what):
    if scale != 4:
        raise NotImplementedError("%s: scale 4 only -- BasicSR's x2 / x1 forms feed the net a pixel-unshuffled input, which is "
                                  "not built (got scale=%r)" % (what, scale))
    if num_features != 64:
        raise NotImplementedError("%s: the dense-block kernels are built for num_features = 64 (got %r)" % (what, num_features))
    if num_grow_ch != 32:
        raise NotImplementedError("%s: the dense-block kernels are built for num_grow_ch = 32 (got %r)" % (what, num_grow_ch))


class RRDBNet(nn.Module):
    """ESRGAN's generator (BasicSR: basicsr/archs/rrdbnet_arch.py RRDBNet), x4."""
    block = RRDB

    def __init__(self, in_features=3, out_features=3, scale=4, num_features=64, num_blocks=23, num_grow_ch=32, **block_args):
        super().__init__()
        _refuse(scale, num_features, num_grow_ch, type(self).__name__)
        self.scale = scale
        self.conv_first = nn.Conv2d(in_features, num_features, 3, 1, 1)
        self.body = nn.Sequential(*[self.block(num_features, num_grow_ch, **block_args) for _ in range(num_blocks)])
        self.conv_body = nn.Conv2d(num_features, num_features, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_features, num_features, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_features, num_features, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_features, num_features, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_features, out_features, 3, 1, 1)

    def _gates(self, metadata):
        return [None] * len(self.body)

    def forward(self, x, metadata=None):
        _check_rgb(x, type(self).__name__)
        if x.dim() != 4 or x.shape[1] != self.conv_first.in_channels:
            raise RuntimeError("%s takes (B, %d, H, W) images; got %s" % (type(self).__name__, self.conv_first.in_channels,
                                                                          tuple(x.shape)))
        gates = self._gates(metadata)
        feat = ops.conv3x3(x, self.conv_first.weight, self.conv_first.bias)
        t = feat
        for blk, m in zip(self.body, gates):
            t = blk(t, m)
        f = ops.conv3x3(t, self.conv_body.weight, self.conv_body.bias, residual=feat)
        f = ops.conv_chain(ops.nearest_up(f, 2), [(self.conv_up1.weight, self.conv_up1.bias, 2)])
        f = ops.conv_chain(ops.nearest_up(f, 2), [(self.conv_up2.weight, self.conv_up2.bias, 2),
                                                  (self.conv_hr.weight, self.conv_hr.bias, 2)])
        return ops.conv3x3(f, self.conv_last.weight, self.conv_last.bias)


class QRRDBNet(RRDBNet):
    """RRDBNet with a meta-attention gate on every RRDB's residual branch (as QEDSR gates its residual blocks)."""
    block = QRRDB

    def __init__(self, in_features=3, out_features=3, scale=4, num_features=64, num_blocks=23, num_grow_ch=32, input_para=1,
                 q_layer_nonlinearity=False, **kwargs):
        super().__init__(in_features, out_features, scale, num_features, num_blocks, num_grow_ch, input_para=input_para,
                         q_layer_nonlinearity=q_layer_nonlinearity)

    def meta_gate_layers(self):
        """The layers forward() hands to meta_gates() in one batch (architectures.late_parameters)."""
        return [b.attention_layer for b in self.body]

    def _gates(self, metadata):
        if metadata is None:
            raise RuntimeError("QRRDBNet needs the metadata of the batch")
        return meta_gates(self.meta_gate_layers(), metadata)


class RRDBHandler(BaseModel):
    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, scale=4, in_features=3, hr_data_loc=None,
                 scheduler=None, scheduler_params=None, perceptual=None, num_features=64, num_blocks=23, num_grow_ch=32,
                 **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, hr_data_loc=hr_data_loc,
                         **kwargs)
        self.net = RRDBNet(in_features=in_features, scale=scale, num_features=num_features, num_blocks=num_blocks,
                           num_grow_ch=num_grow_ch)
        self.colorspace = 'rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.training_setup(lr, scheduler, scheduler_params, perceptual, device)
        self.model_name = 'rrdb'


class QRRDBHandler(QModel):
    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, scale=4, in_features=3, scheduler=None,
                 scheduler_params=None, perceptual=None, num_features=64, num_blocks=23, num_grow_ch=32, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        self.net = QRRDBNet(in_features=in_features, scale=scale, num_features=num_features, num_blocks=num_blocks,
                            num_grow_ch=num_grow_ch, input_para=self.num_metadata, **kwargs)
        self.colorspace = 'augmented_rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.model_name = 'qrrdb'
        self.criterion = L1Loss()
        self.training_setup(lr, scheduler, scheduler_params, perceptual, device)

