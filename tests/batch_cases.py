"""Shape tables and the runner of tests/test_gpu_batch_invariance.py: the per-RoI layer families of the shipped heads as
`hip_ops.ConvLayer`s with random weights, run once on the rows of B images together -- with `dat_conv_desc.plan_frames` = one image's
rows, the hint `workspace.Executor` passes -- and once on each image's rows alone, under the planner's own plans.

Channel counts are those of the shipped heads (tests/model_util.py, configs/): keypoint head 256 / 512 -> 512 on 14 x 14 maps, 17 keypoints,
the C4 res5 head 512 -> 512 3 x 3 x 3 on 7 x 7 maps, the 2-MLP box head 7 * 7 * 256 -> 1024 -> 1024 -> 2 / 8."""
import torch

R_VALUES = (8, 20, 50, 100)             # rows (RoIs) of one image
B_VALUES = (2, 4)                       # images per forward
T_TUBE = 3                              # frames per RoI of the tube heads (configs/test_r18_c4_tube_*.yaml)
K_KPS = 17
SENTINEL = -7.0
SPARE = 3                               # rows behind the last image's segment that a launch must leave untouched

# family -> (kind, parameters).  kind 'conv': input [R * T, H, W, cin], rows on the frames axis; 'fc': input [1, 1, R, cin], rows on W
FAMILIES = {
    'kps_conv3x3_512': dict(kind='conv', cin=512, cout=512, k=(1, 3, 3), pads=(0, 1, 1), hw=14, T=1, relu=True),
    'kps_conv3x3_256': dict(kind='conv', cin=256, cout=512, k=(1, 3, 3), pads=(0, 1, 1), hw=14, T=1, relu=True),
    'c4_res5_3x3x3': dict(kind='conv', cin=512, cout=512, k=(3, 3, 3), pads=(1, 1, 1), hw=7, T=T_TUBE, relu=True),
    'deconv_subpixel': dict(kind='deconv', cin=512, hw=14, T=1),
    'deconv_time_to_channel': dict(kind='deconv', cin=512, hw=14, T=T_TUBE),
    'conv_time_to_channel': dict(kind='conv', cin=512, cout=K_KPS * T_TUBE, k=(T_TUBE, 1, 1), pads=(0, 0, 0), hw=14, T=T_TUBE, relu=False,
                                 out_t=(0, 1)),
    'conv_key_frame': dict(kind='conv', cin=512, cout=512, k=(1, 3, 3), pads=(0, 1, 1), hw=14, T=T_TUBE, relu=True, out_t=(1, 1)),
    'fc6': dict(kind='fc', cin=7 * 7 * 256, cout=1024, relu=True),
    'fc7': dict(kind='fc', cin=1024, cout=1024, relu=True),
    'cls_score': dict(kind='fc', cin=1024, cout=2, relu=False),
    'bbox_pred': dict(kind='fc', cin=1024, cout=8, relu=False),
}

# The R of the one bf16x3 case per family (B = 4)
X3_R = {f: 50 for f in FAMILIES}

# Cases beyond R <= 100: fc6's split-K factor (up to 8 for a deep 1 x 1 layer) does not move while the whole grid -- row tiles of 128 x 8
# cout blocks x 8 splits -- stays within one round of 512 blocks, which holds up to 512 rows; 16-bit only (1 200 x 12 544 inputs, 30 MB)
EXTRA = {'fc6': [(300, 2, 'h16'), (300, 4, 'h16')]}

# (R, B, mode) of each family's table whose batched result is NOT bit-equal to the run alone when the hint is withheld (plan_frames = 0),
# found by running the table on the MI355X (256 CUs).  test_table_can_fail runs these first and asserts that at least one differs.
# Measured over the whole table: the 3 x 3 families differ at most R (the split-K factor and the 128 / 256-position tile both move; the
# tile size alone never changes bits -- with the hint the batched launch often runs 256-position tiles against 128 alone and is equal);
# conv_time_to_channel differs in fp32 and bf16x3 only, fc7 only at 4 x 100 rows in 16 bit.
# A family with an empty list has no such shape for R <= 100 and B <= 4 (cls_score and bbox_pred: 1 to 4 row tiles x one cout block stay far
# inside one round whatever the factor, so the planner picks the same one): only the equality assertion is kept for it.
DIFFERS_WITHOUT_HINT = {
    'kps_conv3x3_512': [(20, 2, 'h16'), (50, 2, 'fp32')],
    'kps_conv3x3_256': [(20, 2, 'h16'), (20, 2, 'fp32')],
    'c4_res5_3x3x3': [(8, 2, 'h16'), (8, 2, 'fp32')],
    'deconv_subpixel': [(50, 2, 'h16'), (50, 2, 'fp32')],
    'deconv_time_to_channel': [(20, 2, 'h16'), (20, 2, 'fp32')],
    'conv_time_to_channel': [(20, 2, 'fp32'), (50, 4, 'bf16x3')],
    'conv_key_frame': [(8, 4, 'h16'), (50, 2, 'fp32')],
    'fc6': [(300, 4, 'h16')],
    'fc7': [(100, 4, 'h16')],
    'cls_score': [],
    'bbox_pred': [],
}


def modes(ops):
    return {'h16': (ops.BF16, ops.H16_DTYPE, False), 'fp32': (ops.F32, torch.float32, False), 'bf16x3': (ops.F32, torch.float32, True)}


_LAYERS = {}


def layer_of(ops, family, mode):
    """The family's ConvLayer in `mode`, built once per process (fc6 packs 12.8 M weights)."""
    if (family, mode) in _LAYERS:
        return _LAYERS[(family, mode)]
    from detectandtrack_amd.workspace import Executor
    f = FAMILIES[family]
    dt, _, x3 = modes(ops)[mode]
    g = torch.Generator().manual_seed(sorted(FAMILIES).index(family) + 1)
    if f['kind'] == 'deconv':
        T = f['T']
        # the [T * C, T * K, 4, 4] ConvTranspose filter as the product turns it into the sub-pixel 3 x 3 conv (workspace.op_ConvTranspose,
        # _deconv_over_time_channels): Cout 4 * T * 17 in a padded channel stride
        w = (torch.randn((T * f['cin'], T * K_KPS, 4, 4), generator=g) / (4.0 * f['cin'] ** 0.5)).cuda()
        w3 = ops.deconv_k4s2_as_conv3x3(Executor.deconv_dense_filter(w, T, 1))
        if T > 1:
            w3 = w3.reshape(w3.shape[0], T, f['cin'], 3, 3).permute(0, 2, 1, 3, 4).contiguous()
        bias = torch.randn(T * K_KPS, generator=g).cuda().repeat(4)
        layer = ops.ConvLayer(w3, None, bias, stride=(1, 1), pads=(0, 1, 1), relu=False, dtype=dt, cin_stride=f['cin'], x3=x3)
        assert layer.cstride > layer.cout
    else:
        k = f['k'] if f['kind'] == 'conv' else (1, 1, 1)
        fan = f['cin'] * k[0] * k[1] * k[2]
        w = (torch.randn((f['cout'], f['cin']) + k, generator=g) / fan ** 0.5).cuda()
        bias = torch.randn(f['cout'], generator=g).cuda()
        layer = ops.ConvLayer(w, None, bias, stride=(1, 1), pads=f.get('pads', (0, 0, 0)), relu=f['relu'], dtype=dt, cin_stride=f['cin'], x3=x3)
    _LAYERS[(family, mode)] = layer
    return layer


def inputs_of(ops, family, R, B, mode):
    """B different images' rows, image i scaled by 1 + 2 i (a leak between images changes values)."""
    f = FAMILIES[family]
    td = modes(ops)[mode][1]
    g = torch.Generator(device='cuda').manual_seed(1000 * R + B)
    if f['kind'] == 'fc':
        shape = (R, f['cin'])
    else:
        shape = (R * f['T'], f['hw'], f['hw'], f['cin'])
    return [(torch.randn(shape, generator=g, device='cuda') * (1.0 + 2.0 * i)).to(td) for i in range(B)]


def _launch(ops, family, layer, x, rows_per_image):
    """One launch over the rows `x` into a sentinel-filled buffer with SPARE rows behind it.  Returns (the rows written, the spare rows)."""
    f = FAMILIES[family]
    if f['kind'] == 'fc':
        rows = x.shape[0]
        buf = torch.full((rows + SPARE, layer.cstride), SENTINEL, dtype=x.dtype, device=x.device)
        layer(x.view(1, 1, rows, x.shape[1]), T=1, out=buf[:rows].view(1, 1, rows, layer.cstride), plan_frames=rows_per_image)
        return buf[:rows], buf[rows:]
    T = f['T']
    out_t = f.get('out_t', (0, 1) if (f['kind'] == 'deconv' and T > 1) else None)
    oframes = x.shape[0] if out_t is None else x.shape[0] // T * out_t[1]
    ho, wo = layer.out_hw(x.shape[1], x.shape[2])
    buf = torch.full((oframes + SPARE, ho, wo, layer.cstride), SENTINEL, dtype=x.dtype, device=x.device)
    layer(x, T=T, out=buf[:oframes], out_t=out_t, plan_frames=rows_per_image)
    return buf[:oframes], buf[oframes:]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def run_case(ops, family, R, B, mode, hint=True):
    """(per image: is its segment of the batched output bit-equal to its run alone?, did every launch leave the spare rows alone?)"""
    layer = layer_of(ops, family, mode)
    xs = inputs_of(ops, family, R, B, mode)
    per_image = xs[0].shape[0]           # frames (R * T) or matrix rows (R) one image contributes: what workspace.Executor passes
    got, spare = _launch(ops, family, layer, torch.cat(xs, dim=0), per_image if hint else 0)
    untouched = bool((spare == SENTINEL).all())
    seg = got.shape[0] // B
    equal = []
    for i, x in enumerate(xs):
        alone, spare = _launch(ops, family, layer, x, 0)
        untouched = untouched and bool((spare == SENTINEL).all())
        assert alone.shape[0] == seg
        equal.append(torch.equal(bits(got[i * seg:(i + 1) * seg]), bits(alone)))
    # (the channels behind Cout are never written: both buffers keep the sentinel there, so whole rows compare)
    assert got.shape[-1] == layer.cout or bool((got[..., layer.cout:] == SENTINEL).all())
    return equal, untouched


def table(family):
    return [(R, B, m) for m in ('h16', 'fp32') for B in B_VALUES for R in R_VALUES] + [(X3_R[family], 4, 'bf16x3')] + EXTRA.get(family, [])
