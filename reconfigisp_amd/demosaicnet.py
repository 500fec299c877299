"""DemosaicNet (demosaic index 04, tools_origin.py:289-308): Gharbi et al. 2016, "Deep Joint Demosaicking and Denoising", Bayer
model, depth 15, width 64, in the layout of the public ``demosaicnet`` package (its ``BayerDemosaick`` module).  The weights are
not distributed with the reference; ``load_demosaicnet`` reads a file (or state dict) the user supplies, checks it against
``LAYOUT`` and folds it into the form the HIP path runs (include/risp.h "DemosaicNet"):

  * pack_mosaic into conv1: on the 1-channel mosaic the 2x2 stride-2 conv of the masked mosaic is a selection,
    W'[o][2dy+dx] = W[o][cfa(dy,dx)][dy][dx]; conv1 o pack is then one 3x3 conv on the space-to-depth planes (RISP_LOAD_UNSHUFFLE2)
    whose weights are W1 W', and the pack's bias enters as the per-border-case table of RISP_EPI_CASEBIAS (conv1's zero padding
    sees no bias, so the table sums only the taps that fall inside the image);
  * BGR out: the rows of ``output`` are permuted;
  * cfa='grbg' (weights trained on a G R / B G mosaic): every kernel is mirrored along x - the network run on the x-mirrored
    mosaic, mirrored back (exact for zero padding and an even W).  Which phase the released weights expect was NOT checked here.

All folds are done in float64 and rounded to fp32 once.  Nothing is trained: the op has no weight gradients.
"""
import torch

CFA_PHASES = ('rggb', 'grbg')

# THE key and shape table of the released layout (the one place to correct if the package's layout differs)
LAYOUT = (
    [('main_processor.pack_mosaic.weight', (4, 3, 2, 2)), ('main_processor.pack_mosaic.bias', (4,))]
    + [kv for i in range(1, 16) for kv in (
        ('main_processor.conv%d.weight' % i, (128 if i == 15 else 64, 4 if i == 1 else 64, 3, 3)),
        ('main_processor.conv%d.bias' % i, (128 if i == 15 else 64,)))]
    + [('residual_predictor.weight', (12, 64, 1, 1)), ('residual_predictor.bias', (12,)),
       ('upsampler.weight', (12, 1, 2, 2)), ('upsampler.bias', (3,)),
       ('fullres_processor.post_conv.weight', (64, 6, 3, 3)), ('fullres_processor.post_conv.bias', (64,)),
       ('fullres_processor.output.weight', (3, 64, 1, 1)), ('fullres_processor.output.bias', (3,))])

# masked-mosaic channel (0 R, 1 G, 2 B) of the RGGB site with row parity dy and column parity dx
RGGB = ((0, 1), (1, 2))


def check_state_dict(sd):
    """Raise ValueError naming the first missing, unexpected or wrongly shaped key; return sd."""
    if not isinstance(sd, dict):
        raise ValueError('DemosaicNet weights: expected a state dict, got %s' % type(sd).__name__)
    want = dict(LAYOUT)
    for key, _ in LAYOUT:
        if key not in sd:
            raise ValueError('DemosaicNet weights: missing key %r' % key)
    for key in sd:
        if key not in want:
            raise ValueError('DemosaicNet weights: unexpected key %r' % key)
    for key, shape in LAYOUT:
        got = tuple(torch.as_tensor(sd[key]).shape)
        if got != shape:
            raise ValueError('DemosaicNet weights: %r has shape %s, expected %s' % (key, got, shape))
    return sd


def _read(src):
    if isinstance(src, dict):
        return src
    sd = torch.load(src, map_location='cpu', weights_only=True)
    if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict):
        sd = sd['state_dict']
    return sd


def mirror_x(sd):
    """The state dict of the x-mirrored network: every kernel flipped along x (the 2x2 pack / upsampler kernels swap columns)."""
    return {k: (v.flip(-1) if k.endswith('.weight') else v) for k, v in sd.items()}


def case_table(w1, bp):
    """(cout, 3, 3) float64: the contribution of pack_mosaic's bias bp through conv1 (w1 (cout,4,3,3)) at border case (cy, cx) of
    RISP_EPI_CASEBIAS (0 first row / column, 1 interior, 2 last) - only the taps that fall inside the image"""
    per_tap = torch.einsum('kotx,o->ktx', w1, bp)                     # (cout, ky, kx)
    valid = ((1, 2), (0, 1, 2), (0, 1))
    t = torch.zeros(w1.shape[0], 3, 3, dtype=w1.dtype)
    for cy in range(3):
        for cx in range(3):
            t[:, cy, cx] = per_tap[:, list(valid[cy])][:, :, list(valid[cx])].sum(dim=(1, 2))
    return t


def fold(sd, cfa='rggb'):
    """The float64 tensors the HIP path runs (CPU): 'conv1.weight' (64,4,3,3) on the space-to-depth planes [R,G1,G2,B],
    'conv1.bias', 'conv1.case' (64,3,3); 'conv{2..15}.weight' / '.bias'; 'rp.weight' (12,64), 'rp.bias'; 'up.weight' (12,4)
    ([dy][dx] flattened), 'up.bias'; 'post.weight' (64,6,3,3), 'post.bias'; 'out.weight' (3,64), 'out.bias' in BGR order."""
    if cfa not in CFA_PHASES:
        raise ValueError("DemosaicNet: cfa must be one of %s, got %r" % (CFA_PHASES, cfa))
    sd = {k: torch.as_tensor(v).detach().to('cpu', torch.float64) for k, v in check_state_dict(sd).items()}
    if cfa == 'grbg':
        sd = mirror_x(sd)
    mp = 'main_processor.'
    wp, bp = sd[mp + 'pack_mosaic.weight'], sd[mp + 'pack_mosaic.bias']
    sel = torch.stack([wp[:, RGGB[dy][dx], dy, dx] for dy in range(2) for dx in range(2)], dim=1)    # (4 out, 4 planes)
    w1 = sd[mp + 'conv1.weight']
    out = {'conv1.weight': torch.einsum('kotx,oq->kqtx', w1, sel), 'conv1.bias': sd[mp + 'conv1.bias'],
           'conv1.case': case_table(w1, bp)}
    for i in range(2, 16):
        out['conv%d.weight' % i], out['conv%d.bias' % i] = sd[mp + 'conv%d.weight' % i], sd[mp + 'conv%d.bias' % i]
    out['rp.weight'], out['rp.bias'] = sd['residual_predictor.weight'][:, :, 0, 0], sd['residual_predictor.bias']
    out['up.weight'], out['up.bias'] = sd['upsampler.weight'].reshape(12, 4), sd['upsampler.bias']
    out['post.weight'], out['post.bias'] = sd['fullres_processor.post_conv.weight'], sd['fullres_processor.post_conv.bias']
    out['out.weight'] = sd['fullres_processor.output.weight'][:, :, 0, 0].flip(0)                     # RGB -> BGR rows
    out['out.bias'] = sd['fullres_processor.output.bias'].flip(0)
    return out


class DemosaicNet:
    """A loaded network: the folded fp32 weights, packed for the convolution kernels per device on first use
    (``packs(device)``; call it once before capturing a graph - the first call copies the weights to the device)."""

    def __init__(self, folded, cfa='rggb'):
        self.cfa = cfa
        self.folded = {k: v.float().contiguous() for k, v in folded.items()}
        self._packs = {}

    def packs(self, device):
        key = torch.device(device)
        p = self._packs.get(key)
        if p is None:
            from .convnets import build_demosaicnet_packs
            p = self._packs[key] = build_demosaicnet_packs(self.folded, key)
        return p

    def __call__(self, x, record=None):
        from .functional import demosaicnet
        return demosaicnet(x, self, record)


def load_demosaicnet(src, cfa='rggb'):
    """The packed DemosaicNet from ``src`` (a path to a torch-saved state dict, or the dict itself) in the released layout
    (``LAYOUT``); ``cfa``: 'rggb' uses the weights as they are, 'grbg' mirrors the network along x (weights trained on a
    G R / B G mosaic).  Every key and shape is checked; the error names the offending key."""
    return DemosaicNet(fold(_read(src), cfa), cfa)
