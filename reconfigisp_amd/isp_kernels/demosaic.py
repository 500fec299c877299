"""demosaic.Demosaic - options 'nearestneighbor' (NCHW in/out, tools_origin.py:278-284),
'bilinear' / 'laplacian' (NHWC, 0..255 domain, :457-468, :491-502) and 'demosaicnet' (:302-308)."""
from .. import functional as F
from ._layout import to_nchw, to_nhwc


_DEMOSAICNET = None
_BUILTIN = None             # the network load_demosaicnet registered (None: none, or replaced by register_demosaicnet)


def register_demosaicnet(fn):
    """Plug a user-supplied differentiable DemosaicNet: fn((N,1,H,W) RGGB in [0,1]) -> (N,3,H,W) BGR.
    The original lives only in the private ISP_Kernels package and is not reproducible."""
    global _DEMOSAICNET, _BUILTIN
    _DEMOSAICNET, _BUILTIN = fn, None


def load_demosaicnet(src, cfa='rggb'):
    """Register the built-in DemosaicNet (HIP, include/risp.h) with the weights in ``src`` (a path or a state dict in the layout
    of reconfigisp_amd.demosaicnet.LAYOUT); returns the loaded network.  A later register_demosaicnet(fn) replaces it."""
    global _DEMOSAICNET, _BUILTIN
    from ..demosaicnet import load_demosaicnet as _load
    net = _load(src, cfa)
    _DEMOSAICNET, _BUILTIN = net, net
    return net


def unregister_demosaicnet():
    """Back to no implementation: 'demosaicnet' raises and the super-net masks the op out again."""
    global _DEMOSAICNET, _BUILTIN
    _DEMOSAICNET, _BUILTIN = None, None


def demosaicnet_available():
    return _DEMOSAICNET is not None


class Demosaic:
    def run(self, img, option, params):
        fmt_in = params.get('input', {}).get('format', 'RGGB')
        if fmt_in != 'RGGB':
            raise ValueError('Demosaic: only the RGGB mosaic is supported, got %r' % (fmt_in,))
        if option == 'nearestneighbor':
            return F.demosaic_nearest(img)
        if option in ('bilinear', 'laplacian'):
            return to_nhwc(F.origin_demosaic(to_nchw(img), option))
        if option == 'demosaicnet':
            if _BUILTIN is not None:
                return _BUILTIN(img, params.get('reuse_record'))      # step-level reuse record of the super-net, if any
            if _DEMOSAICNET is not None:
                return _DEMOSAICNET(img)
            raise NotImplementedError(
                "Demosaic 'demosaicnet': the Gharbi-style network and its weights live only in the private "
                'ISP_Kernels package and cannot be reproduced (SURVEY.md section 2); the registry slot is kept')
        raise ValueError('Demosaic: unknown option %r' % (option,))
