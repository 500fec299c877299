"""OriginUniversal - fixed ISP that uses the classical kernels where they exist; only BM3D and the
two Path-Restore nets are learned (mirror of models/modules/origin_universal.py:9-165).  BM3D is classical too
with ``classical_bm3d=True`` (options key ``network_G.classical_bm3d``, off by default).

The shipped reference puts an *instance* ``GtmManual(4)`` into its class pool (:61) and crashes
with TypeError when sRGB index 14 is selected; the documented behaviour (a 4-segment tone curve)
is what is built here."""
from . import registry as R
from .isp_universal import _FixedPipeline


class OriginUniversal(_FixedPipeline):
    srgb_names = R.NAMES_SRGB
    use_origin_kernels = True

    def __init__(self, module_path, architecture, classical_bm3d=False):
        """classical_bm3d: sRGB index 15 runs the classical BM3D kernels (OriginNoiseBm3d) instead of the proxy"""
        super().__init__()
        self._build(module_path, architecture, classical_bm3d=classical_bm3d)
