"""Spatial / temporal discriminators (mirror of dgmr/discriminators.py) on the HIP operators."""
import torch
from huggingface_hub import PyTorchModelHubMixin

from . import ops
from .common import DBlock
from .nn import BatchNorm1d, SNLinear1, SNScope


class Discriminator(torch.nn.Module, PyTorchModelHubMixin):
    """dgmr/discriminators.py:12-44."""

    def __init__(self, input_channels: int = 12, num_spatial_frames: int = 8, conv_type: str = "standard"):
        super().__init__()
        self.spatial_discriminator = SpatialDiscriminator(input_channels=input_channels, num_timesteps=num_spatial_frames,
                                                          conv_type=conv_type)
        self.temporal_discriminator = TemporalDiscriminator(input_channels=input_channels, conv_type=conv_type)

    def forward(self, x: torch.Tensor, calls: int = 1) -> torch.Tensor:
        """`calls` > 1: x stacks the inputs of `calls` consecutive calls of the reference's discriminator ([calls * N, T, C, H, W]:
        the generator pass scores each of its draws with a separate call, dgmr/dgmr.py:186-193).  Each call keeps its own random
        frame draw, spectral-norm sigmas and BatchNorm1d batch statistics, all advanced in call order."""
        if x.shape[0] % calls:
            raise RuntimeError(f"discriminator: batch {x.shape[0]} is not divisible into {calls} calls")
        # (ops.set_precision: the discriminator forward may run in a finer arithmetic mode than the rest of the step)
        with ops.discriminator_forward_precision(), SNScope(self, (tuple(x.shape), calls)):  # all spectral-norm iterations up front
            spatial_loss = self.spatial_discriminator(x, calls=calls)
            temporal_loss = self.temporal_discriminator(x, calls=calls)
        return torch.cat([spatial_loss, temporal_loss], dim=1)

    def forward_split(self, context: torch.Tensor, real: torch.Tensor, generated: torch.Tensor, calls: int = 1) -> torch.Tensor:
        """forward(x, calls) for x = [call][cat(context, real) | cat(context, generated[call])] - the generator pass's `calls`
        discriminator calls on cat(real, draw) (dgmr/dgmr.py:186-193) - without building x: context [B, Tc, C, H, W] and real
        [B, T, C, H, W] are shared by the calls, generated is [calls * B, T, C, H, W].  Same scores, same state afterwards and the same
        gradient for `generated`, bit for bit; the difference is what is NOT done.  The real sequences have to run forward (each call's
        BatchNorm1d takes its batch statistics over real and generated rows together), but nothing reads their backward when the
        discriminator's parameters are frozen: below the BatchNorm1d heads no operator couples the samples of a batch.  So every
        block runs as two launch sets - real under no_grad (nothing saved), generated with a graph - that read the same spectral-norm
        records (the state advances once per call) and run the kernels the joint batch would get (ops.ConvSpec.plan_mult); the
        halves meet in the joint row order in front of the heads, which run unchanged.  Needs an even B (the 8x8 maps' two-image
        tiles must not straddle two calls) and a discriminator whose parameters take no gradient from this call."""
        b = context.shape[0]
        if generated.shape[0] != calls * b or real.shape[0] != b or b % 2:
            raise RuntimeError(f"discriminator: {tuple(generated.shape)} generated and {tuple(real.shape)} real sequences do not make "
                               f"{calls} calls on an even batch of {b}")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("discriminator: forward_split computes no parameter gradients; freeze the parameters or use forward()")
        shape = (2 * calls * b, context.shape[1] + real.shape[1]) + tuple(context.shape[2:])  # (of the joint batch: one plan for both entries)
        with ops.discriminator_forward_precision(), SNScope(self, (shape, calls)):
            spatial_loss = self.spatial_discriminator.forward_split(context, real, generated, calls=calls)
            temporal_loss = self.temporal_discriminator.forward_split(context, real, generated, calls=calls)
        return torch.cat([spatial_loss, temporal_loss], dim=1)


def _both(block, xr, xg, calls: int, layout=None):
    """One forward of a DBlock on a batch that exists as its real (no graph) and generated halves."""
    sn = block.draw_sn(calls, layout)
    with torch.no_grad():
        yr = block(xr, calls=calls, layout=layout, sn=sn, plan_mult=2)
    return yr, block(xg, calls=calls, layout=layout, sn=sn, plan_mult=2)


def _joint_heads(bn, fc, rr, rg, groups: int, layout, frames: int):
    """relu + sum over the map per half, then BatchNorm1d -> linear -> sum over the frames on the joint [group][real | generated] rows."""
    with torch.no_grad():
        fr = ops.relu_sum_hw(rr)
    rep = ops.interleave_halves(fr, ops.relu_sum_hw(rg), groups)
    rep = bn(rep, groups=groups, layout=layout)
    rep = fc(rep, calls=groups, layout=layout)
    return _sum_heads(rep, frames)


def _sum_heads(reps, frames):
    return ops.sum_groups(reps, frames).unsqueeze(1)  # [frames*N, 1] -> [N, 1, 1]


def _frame_layout(calls: int, frames: int):
    """Groups of a frame-major batch that stacks `calls` discriminator calls: [frame][call]; reference order: call-major."""
    return ops.CallLayout(calls, frames, time_major=True) if calls > 1 else None


class TemporalDiscriminator(torch.nn.Module, PyTorchModelHubMixin):
    """dgmr/discriminators.py:47-138."""

    def __init__(self, input_channels: int = 12, num_layers: int = 3, conv_type: str = "standard"):
        super().__init__()
        self.downsample = torch.nn.AvgPool3d(kernel_size=(1, 2, 2), stride=(1, 2, 2))
        self.space2depth = torch.nn.PixelUnshuffle(downscale_factor=2)
        internal_chn = 48
        self.d1 = DBlock(4 * input_channels, internal_chn * input_channels, conv_type="3d", first_relu=False)
        self.d2 = DBlock(internal_chn * input_channels, 2 * internal_chn * input_channels, conv_type="3d")
        self.intermediate_dblocks = torch.nn.ModuleList()
        for _ in range(num_layers):
            internal_chn *= 2
            self.intermediate_dblocks.append(
                DBlock(internal_chn * input_channels, 2 * internal_chn * input_channels, conv_type=conv_type))
        self.d_last = DBlock(2 * internal_chn * input_channels, 2 * internal_chn * input_channels, keep_same_output=True,
                             conv_type=conv_type)
        self.fc = SNLinear1(2 * internal_chn * input_channels)
        self.relu = torch.nn.ReLU()
        self.bn = BatchNorm1d(2 * internal_chn * input_channels)

    def forward(self, x: torch.Tensor, calls: int = 1) -> torch.Tensor:
        ops.require_hip(x, "discriminator frames")
        # AvgPool3d((1,2,2)) + PixelUnshuffle(2) + permute to N C T H W, written once as N T H W C
        x = ops.frames_s2d(x, None, pool=True, frame_major=False, as_3d=True)
        x = self.d1(x, calls=calls)  # the 3-D blocks run once per discriminator call: groups are already in call order
        x = self.d2(x, calls=calls)
        # the reference loops over the remaining frames (discriminators.py:119-133); here they form one frame-major batch and
        # every block / head runs once, each frame keeping its own spectral-norm sigma and BatchNorm1d batch statistics
        frames = x.size(2)
        lay = _frame_layout(calls, frames)
        groups = frames * calls
        rep = ops.frames_to_batch(x)
        for d in self.intermediate_dblocks:
            rep = d(rep, calls=groups, layout=lay)
        rep = self.d_last(rep, calls=groups, layout=lay)
        rep = ops.relu_sum_hw(rep)
        rep = self.bn(rep, groups=groups, layout=lay)
        rep = self.fc(rep, calls=groups, layout=lay)
        return _sum_heads(rep, frames)

    def forward_split(self, context, real, generated, calls: int = 1) -> torch.Tensor:
        """Discriminator.forward_split: `forward` on the joint batch, run as its real and generated halves."""
        ops.require_hip(generated, "discriminator frames")
        n = generated.shape[0]
        with torch.no_grad():
            xr = ops.frames_s2d_pair(context, real, None, n=n, pool=True, frame_major=False, as_3d=True)
        xg = ops.frames_s2d_pair(context, generated, None, n=n, pool=True, frame_major=False, as_3d=True)
        xr, xg = _both(self.d1, xr, xg, calls)
        xr, xg = _both(self.d2, xr, xg, calls)
        frames = xg.size(2)
        lay = _frame_layout(calls, frames)
        groups = frames * calls
        with torch.no_grad():
            rr = ops.frames_to_batch(xr)
        rg = ops.frames_to_batch(xg)
        for d in list(self.intermediate_dblocks) + [self.d_last]:
            rr, rg = _both(d, rr, rg, groups, lay)
        return _joint_heads(self.bn, self.fc, rr, rg, groups, lay, frames)


class SpatialDiscriminator(torch.nn.Module, PyTorchModelHubMixin):
    """dgmr/discriminators.py:141-232."""

    def __init__(self, input_channels: int = 12, num_timesteps: int = 8, num_layers: int = 4, conv_type: str = "standard"):
        super().__init__()
        self.num_timesteps = num_timesteps
        self.mean_pool = torch.nn.AvgPool2d(2)
        self.space2depth = torch.nn.PixelUnshuffle(downscale_factor=2)
        internal_chn = 24
        self.d1 = DBlock(4 * input_channels, 2 * internal_chn * input_channels, first_relu=False, conv_type=conv_type)
        self.intermediate_dblocks = torch.nn.ModuleList()
        for _ in range(num_layers):
            internal_chn *= 2
            self.intermediate_dblocks.append(
                DBlock(internal_chn * input_channels, 2 * internal_chn * input_channels, conv_type=conv_type))
        self.d6 = DBlock(2 * internal_chn * input_channels, 2 * internal_chn * input_channels, keep_same_output=True,
                         conv_type=conv_type)
        self.fc = SNLinear1(2 * internal_chn * input_channels)
        self.relu = torch.nn.ReLU()
        self.bn = BatchNorm1d(2 * internal_chn * input_channels)

    def forward(self, x: torch.Tensor, calls: int = 1) -> torch.Tensor:
        ops.require_hip(x, "discriminator frames")
        # frame indices come from the CPU generator exactly as in the reference (discriminators.py:199): one draw per call
        idxs = torch.stack([torch.randint(low=0, high=x.size()[1], size=(self.num_timesteps,)) for _ in range(calls)])
        idxs_dev = ops.upload(idxs, x.device, torch.int32)  # (asynchronous: the host does not wait for the queue to drain)
        frames = self.num_timesteps
        lay = _frame_layout(calls, frames)
        groups = frames * calls
        # AvgPool2d(2) + PixelUnshuffle(2) of the drawn frames, frame-major: the reference's per-frame loop
        # (discriminators.py:201-226) as one batch of `frames` calls per block
        rep = ops.frames_s2d(x, idxs_dev, pool=True, frame_major=True, idx_group=x.shape[0] // calls)
        rep = self.d1(rep, calls=groups, layout=lay)
        for d in self.intermediate_dblocks:
            rep = d(rep, calls=groups, layout=lay)
        rep = self.d6(rep, calls=groups, layout=lay)
        rep = ops.relu_sum_hw(rep)
        rep = self.bn(rep, groups=groups, layout=lay)
        rep = self.fc(rep, calls=groups, layout=lay)
        return _sum_heads(rep, frames)

    def forward_split(self, context, real, generated, calls: int = 1) -> torch.Tensor:
        """Discriminator.forward_split: `forward` on the joint batch, run as its real and generated halves (one frame draw per call,
        from the CPU generator in call order, read by both)."""
        ops.require_hip(generated, "discriminator frames")
        n = generated.shape[0]
        steps = context.shape[1] + real.shape[1]
        idxs = torch.stack([torch.randint(low=0, high=steps, size=(self.num_timesteps,)) for _ in range(calls)])
        idxs_dev = ops.upload(idxs, generated.device, torch.int32)
        frames = self.num_timesteps
        lay = _frame_layout(calls, frames)
        groups = frames * calls
        with torch.no_grad():
            rr = ops.frames_s2d_pair(context, real, idxs_dev, n=n, pool=True, frame_major=True, idx_group=n // calls)
        rg = ops.frames_s2d_pair(context, generated, idxs_dev, n=n, pool=True, frame_major=True, idx_group=n // calls)
        for d in [self.d1] + list(self.intermediate_dblocks) + [self.d6]:
            rr, rg = _both(d, rr, rg, groups, lay)
        return _joint_heads(self.bn, self.fc, rr, rg, groups, lay, frames)
