"""IspUniversal - a fixed ISP built from an architecture string, proxy variant.

Host-side mirror of models/modules/isp_universal.py:12-236: same constructor arguments,
``forward``, ``trainable_parameters``, ``intermediate_results`` and state-dict keys
(``param_step<k>_<name>``).  Differences from the shipped reference, both documented in
SURVEY.md: the reference crashes at construction on undefined names (:92-94) - here pool
entries 19-21 raise only when selected; inference forwards run fused (pipeline_fusion.py).
"""
import numpy as np
import torch
import torch.nn as nn

from .... import functional as F
from . import registry as R
from .pipeline_fusion import fused_forward, output_plan, serve_frame_reported, serve_reported, stats_plan, temporal_plan, wants_grad


class _FixedPipeline(nn.Module):
    """Shared machinery of IspUniversal / OriginUniversal."""
    srgb_names = R.NAMES_SRGB
    use_origin_kernels = False

    def _build(self, module_path, architecture, indiv_module_paths=None, conditional=None, classical_bm3d=False):
        conditional = conditional or {}
        self.architecture = architecture
        self.all_modules, self.all_params, self.is_conditional, self.step_names = [], [], [], []
        for step, (_, name) in enumerate(R.parse_architecture(architecture, self.srgb_names), start=1):
            override = indiv_module_paths[step - 1] if indiv_module_paths is not None and name in R.PROXY_NETS else None
            cond_ch = conditional.get(R.CONDITIONAL_KW.get(name))
            op = R.make_op(name, module_path, origin=self.use_origin_kernels, weight_override=override,
                           conditional_channels=cond_ch, classical_bm3d=classical_bm3d)
            init = list(R.PARAM_INIT[name])
            if name in R.CONDITIONAL_KW:
                # FC weights ~ N(0, 0.01^2), then the 'global' module parameters (isp_universal.py:185-190)
                init = list(np.random.randn(op.total_params - len(init)) * 0.01) + init
            self.all_modules.append(op)
            self.is_conditional.append(name in R.CONDITIONAL_KW)
            self.step_names.append(name)
            if init:
                key = 'param_step{}_{}'.format(step, name)
                setattr(self, key, nn.Parameter(torch.tensor(init, dtype=torch.float32)))
                self.all_params.append(getattr(self, key))
            else:
                self.all_params.append(nn.Parameter(torch.zeros(0)))
        self.intermediate_results = []
        self.last_serve_route = None            # 'fused' | 'classical' | 'scene' | 'denoise' (a median of size 5 .. 15 under fast_median too) | 'denoise_scene' | 'cond' | 'composed' | 'tiled' (serve_frame): what the last serve call ran
        self.last_serve_store = None            # with out_format='nv12': 'fused' (the serving launch stored NV12) | 'pass' (the conversion launch did) | 'resize' (with out_size / out_window: the resize launch did); None for 'bgr8'
        self.last_serve_resize = None           # with out_size / out_window: 'pass' (risp_bgr8_resize behind the route); None without the keywords
        self.last_serve_shade = None            # with lens_shading: 'fused' (the serving launch shaded in its load) | 'pass' (risp_raw_shade did, decoding packed frames too); None without the keyword
        self.last_serve_defect = None           # with defect_correction: 'fused' (one risp_raw_defect launch corrected and shaded) | 'pass' (risp_raw_defect corrected; risp_raw_shade follows where lens_shading is given); None without the keyword
        self.last_serve_sharpen = None          # with sharpen: 'pass' (risp_bgr8_sharpen behind the route, the warp and the resize); None without the keyword
        self.last_serve_warp = None             # with warp: 'pass' (risp_bgr8_warp behind the route); None without the keyword
        self.last_serve_temporal = None         # with temporal_denoise: 'pass' (risp_raw_temporal filtered the frames in front of the route and advanced the state); None without the keyword
        self.last_serve_stats = None            # with statistics: 'pass' (risp_raw_stats filled the RawStatistics from what the route reads); None without the keyword
        self.last_serve_load = None             # with raw_format='raw10' / 'raw12': 'fused' (the serving launch decoded the packed bytes) | 'pass' (the unpack launch did); None for 'u16'

    def _apply(self, fn, *args, **kwargs):
        # sub-modules and zero-size placeholders live in plain lists (as in the reference, so the
        # state dict holds only param_step*); unlike the reference they still follow .to()/.cuda()
        super()._apply(fn, *args, **kwargs)
        for m in self.all_modules:
            m._apply(fn, *args, **kwargs)
        for p in self.all_params:
            if p.numel() == 0:
                p.data = fn(p.data)
        return self

    def _stage_params(self, n):
        if not torch.is_grad_enabled():
            # inference: sigmoid(p).repeat(N,1) only changes when a parameter does - keep the (N,P)
            # blocks resident instead of re-launching 2 tiny kernels per stage per call
            key = (n,) + tuple((p._version, p.data_ptr()) for p in self.all_params)
            if getattr(self, '_stage_cache_key', None) != key:
                self._stage_cache, self._stage_cache_key = self._build_stage_params(n), key
            return self._stage_cache
        return self._build_stage_params(n)

    def _build_stage_params(self, n):
        plain = [p for p, cond in zip(self.all_params, self.is_conditional) if p.numel() and not cond]
        blocks = iter(F.param_blocks(plain, n))                # sigmoid(p).repeat(n, 1), (N, P) in [0,1]: one launch
        out = []
        for p, cond in zip(self.all_params, self.is_conditional):
            if p.numel() == 0:
                out.append(None)
            elif cond:
                out.append(p)                                  # raw flat vector, no sigmoid / repeat
            else:
                out.append(next(blocks))
        return out

    def forward(self, x):
        pars = self._stage_params(x.size(0))
        # segment fusion works on 2 x 4 pixel patches: odd sizes (sRGB-only pipelines may see them) go op by op
        if x.is_cuda and not wants_grad(x, self.all_params) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0:
            with torch.no_grad():
                # (final_out: set by test_split.run_frame around model.test() - the last stage written into the frame's tile stack)
                x, self.intermediate_results = fused_forward(self.all_modules, pars, x, self.__dict__.get('final_out'))
            return x
        self.intermediate_results = []
        for op, par in zip(self.all_modules, pars):
            x = op(x, par)
            self.intermediate_results.append(x)
        return x

    def serve(self, raw_u16, white_level, reverse_channels=False, out=None, black_level=0, cfa='rggb', fast_scene=False,
              fast_denoise=False, fast_cond=False, *, sharpen=None, out_format='bgr8', yuv_matrix='bt601_full', out_size=None, out_window=None,
              resample='triangle', raw_format='u16', temporal_denoise=None, statistics=None, warp=None, raw_width=None,
              lens_shading=None, defect_correction=None, fast_median=False, fast_denoise_scene=False):
        """The pipeline as an ISP: (N,H,W) uint16 RGGB frames on the device -> (N,H,W,3) uint8, the bytes of
        ``tensor2bgr(self(raw / white_level))`` image by image (RGB order with ``reverse_channels``).  One launch where
        ``pipeline_fusion.serve_route`` says 'fused' (and the learned bilateral window allows it) or 'classical' (a classical
        bilinear / Malvar-He-Cutler demosaic, Crysis / Filmic tone curves), otherwise composed from the existing kernels;
        ``last_serve_route`` records the route taken.  ``intermediate_results`` is left as it was.  ``black_level`` and ``cfa`` ('rggb' | 'grbg' | 'gbrg'
        | 'bggr') describe the sensor (``pipeline_fusion.serve``): the pedestal is subtracted in integers, the divisor is
        white_level - black_level, and another phase is served by mirrored addresses, without a further pass.

        ``fast_scene=True`` opts a pipeline with one or two of gray-world, white-world, Reinhard in to the ``'scene'`` route
        (``pipeline_fusion.scene_plan``; H even and >= 4, W % 4 == 0): 2 S + 1 launches for S scene stages, the mosaic read
        again per statistic instead of fp32 planes written.  White-world-only pipelines keep the composed route's bytes;
        gray-world and Reinhard sum in another order and agree with the float64 reference of
        tests/serve_scene_reference.py under its tie rule, not byte for byte.  Where the route does not apply the call runs
        as without the flag.

        ``fast_denoise=True`` opts a pipeline with one classical bilateral, median or non-local means behind a classical
        demosaic in to the ``'denoise'`` route (``pipeline_fusion.denoise_plan``; H even and >= 4, W % 4 == 0, learned sizes
        3 / 3 / (3, 3)): one launch with the composed route's bytes.  Where the route does not apply the call runs as
        without the flag.

        ``fast_median=True`` opts a pipeline with one classical median of ANY learned size below a saturated parameter in to that
        route (``pipeline_fusion._median_args``: 2 * int(p * 7) + 3 from image 0's parameter): size 3 takes the launch above, a
        size in ``pipeline_fusion._MEDIAN_SIZES`` with min(H, W) > size // 2 takes ``risp_serve_median_u8`` - one launch, the
        composed route's bytes, ``last_serve_route`` 'denoise'.  Where it does not apply (size 17, any other denoiser) the
        call runs as without the flag.

        ``fast_cond=True`` opts a pipeline with one to three conditional heads (ConditionalGamma / ConditionalWbManual /
        ConditionalWbQuadratic) among element-wise stages and Crysis / Filmic curves behind a classical demosaic in to the
        ``'cond'`` route (``pipeline_fusion.cond_plan``; H even and >= 4, W % 4 == 0, H * W <= 2^24): 2 S + 1 launches for S
        heads, the mosaic read again per histogram instead of fp32 planes written, with the composed route's bytes.  Where
        the route does not apply the call runs as without the flag.

        ``fast_denoise_scene=True`` opts a pipeline with one classical bilateral, median or non-local means AND one or two of
        gray-world / white-world behind a classical demosaic in to the ``'denoise_scene'`` route
        (``pipeline_fusion.denoise_scene_plan``; H even and >= 4, W % 4 == 0, learned sizes 3 / 3 / (3, 3)): 2 S + 1 launches
        for S scene stages, no fp32 plane written.  White-world-only lists keep the default call's bytes; with gray-world the
        bytes are the composed route's for the same gains, and the gains are within the summation bound of the composed
        route's.  Where the route does not apply the call runs as without the flag.

        ``out_format='nv12'`` returns (N,3H/2,W) YUV 4:2:0 - H rows of Y, H/2 rows of interleaved U V, ``yuv_matrix`` a key of
        ``functional.NV12_MATRIX`` or twelve integers -, byte for byte ``functional.bgr8_to_nv12`` of the same call's BGR
        bytes, on the route the call takes without the keyword.  ``last_serve_store`` records who stored it: 'fused' (the one
        launch of the 'fused' / 'classical' route) or 'pass' (``risp_bgr8_to_nv12`` behind any other route); None for 'bgr8'.
        H and W even; ``reverse_channels`` is refused.

        ``raw_format='raw10'`` / ``'raw12'`` takes the frames MIPI-packed, (N,H,stride) uint8 with ``raw_width`` pixels per row
        (None: all the rows hold) - the bytes of the same call on ``functional.raw_unpack`` of them, on the same route.
        ``last_serve_load`` records who decoded them, as ``pipeline_fusion.serve_load`` tells: 'fused' (the one launch of the
        'fused' / 'classical' route) or 'pass' (``risp_raw_unpack`` in front of any other route); None for 'u16'.
        ``white_level`` is not implied by the format.

        ``lens_shading=(gains, cell)`` corrects vignetting and colour shading in front of everything else: (GH,GW,4) uint16 Q12
        gains on the device on a mesh of ``cell`` pixels (``functional.shading_map`` builds one; include/risp.h has the integer
        definition) - the bytes of the same call on ``functional.raw_shade(frames, lens_shading, black_level)`` with
        ``white_level - black_level`` and black level 0, on the same route.  ``last_serve_shade`` records who shaded, as
        ``pipeline_fusion.serve_shade`` tells: 'fused' (the one launch of the 'classical' route, 8-byte aligned uint16 frames)
        or 'pass' (``risp_raw_shade`` in front of the route, which decodes packed frames too: ``last_serve_load`` is then
        'pass'); None without the keyword.

        ``defect_correction=(threshold, slope, defects)`` replaces hot, dead and factory-listed pixels from their same-colour
        neighbours in front of everything else (``functional.defect_check``, ``functional.defect_map``; include/risp.h has the
        integer definition) - the bytes of the same call on ``functional.raw_defect(frames, defect_correction, bits, raw_width)``
        as uint16 input, with ``lens_shading`` on ``functional.raw_shade`` of those, on the route that call takes.  One
        ``risp_raw_defect`` launch in front of the route, which decodes packed frames too (``last_serve_load`` is then 'pass',
        ``last_serve_shade`` 'pass' with a shading).  ``last_serve_defect`` records the pre-pass as
        ``pipeline_fusion.defect_shade`` tells: 'fused' (that one launch shaded as well) or 'pass' (it corrected alone;
        ``risp_raw_shade`` follows where a shading is given); None without the keyword.

        ``temporal_denoise=(state, strength, threshold, slope, ramp)`` filters the frames over time behind those pre-passes and
        in front of the statistics and the route: each sample is blended over ``state.frames`` (a ``functional.TemporalState``,
        built once by ``functional.temporal_state``) with a Q8 share that starts at ``strength`` and climbs to 256 where the
        5 x 5 neighbourhood moved (``functional.temporal_check``; include/risp.h has the integer definition) - the bytes of the
        same call without the keyword on ``functional.raw_temporal`` of the pre-pass's frames, on the route that call takes, and
        the state advanced to those frames.  One ``risp_raw_temporal`` launch and one copy; packed frames without a pre-pass are
        unpacked first (``last_serve_load`` is then 'pass', ``last_serve_shade`` 'pass' with a shading).  An unprimed state is
        primed by the call - refused while the stream is capturing; a primed call with ``out`` captures, and every replay
        advances the state.  ``last_serve_temporal`` is 'pass', None without the keyword.

        ``out_size=(OH, OW)`` and ``out_window=(y0, x0, h, w)`` deliver a scaled, cropped image (N,OH,OW,3): the window of the
        image as returned (default: all of it) resampled to ``out_size`` (default: the window's size, a crop) with ``resample``
        'box', 'triangle' or 'bicubic' - the bytes of ``functional.bgr8_resize`` of the same call without the keywords, on the
        route that call takes (include/risp.h has the integer definition).  The route serves packed BGR into a cached image
        and one ``risp_bgr8_resize`` launch writes ``out``: ``last_serve_resize`` is 'pass', None without the keywords.  With
        ``out_format='nv12'`` (N,3*OH/2,OW), OH and OW even; ``last_serve_store`` is then 'resize' (that launch stored NV12,
        where ``pipeline_fusion.resize_store`` says 'fused') or 'pass' (``risp_bgr8_to_nv12`` followed it).  ``out_format``,
        ``yuv_matrix``, ``out_size``, ``out_window``, ``resample``, ``raw_format``, ``temporal_denoise``, ``statistics``, ``warp``, ``raw_width``,
        ``lens_shading``, ``defect_correction``, ``fast_median`` and ``fast_denoise_scene`` are keyword-only
        (``pipeline_fusion.serve``).

        ``statistics=st`` (a ``functional.RawStatistics``, built once by ``functional.raw_statistics``) also fills ``st.zones``
        and ``st.hist`` with the 3A statistics of the samples the route demosaics - zone sums and counts, the focus measure,
        histograms; include/risp.h has the integer definition.  ``st`` is checked before anything is launched, then
        ``risp_raw_stats`` reads what the route is about to read: the pre-pass's frames with ``defect_correction`` and / or
        ``lens_shading`` (the shade launch then runs: ``last_serve_shade`` 'pass'), otherwise the input as given.  The image
        bytes and the route are those of the call without the keyword.  ``last_serve_stats`` is 'pass', None without it.

        ``warp=(mesh, cell, (WH, WW), kernel)`` delivers a geometry-corrected image (N,WH,WW,3): lens distortion, rotation,
        flips, keystone, stabilisation through an (MH,MW,2) int32 mesh of Q8 source coordinates with 'bilinear' or 'bicubic'
        taps (``functional.warp_check``; ``functional.warp_mesh`` / ``warp_homography`` / ``warp_radial`` build meshes;
        include/risp.h has the integer definition).  The route, chosen as without the keyword, serves packed BGR into a cached
        image and one ``risp_bgr8_warp`` launch writes the warped image - into ``out``, or in front of the resize
        (``out_size`` / ``out_window`` then apply to the warped image) and of the NV12 conversion (WH, WW even;
        ``last_serve_store`` 'pass' or as under a resize): the bytes of ``functional.bgr8_warp`` of the same call without the
        keyword.  Statistics are unchanged.  ``last_serve_warp`` is 'pass', None without it.

        ``sharpen=(amount, threshold, limit, radius)`` (keyword-only) sharpens the image as returned, behind ``warp`` and
        ``out_size`` / ``out_window`` and in front of the NV12 conversion: an unsharp mask of the 8-bit luma - binomial blur of
        ``radius`` 1 or 2, soft coring by ``threshold`` codes, the gain ``amount`` / 256 (0 .. 4095), at most ``limit`` codes -
        added to B, G and R alike (``functional.sharpen_check``; include/risp.h has the integer definition).  The stage in front
        of it stores packed BGR into a cached image and one ``risp_bgr8_sharpen`` launch writes ``out``: the bytes of
        ``functional.bgr8_sharpen`` of the same call without the keyword, ``reverse_channels`` honoured.  With
        ``out_format='nv12'`` ``last_serve_store`` is 'sharpen' (that launch stored NV12, where
        ``pipeline_fusion.sharpen_store`` says 'fused') or 'pass' (``risp_bgr8_to_nv12`` followed it).  Statistics, the temporal
        state and every other ``last_serve_*`` are unchanged.  ``last_serve_sharpen`` is 'pass', None without it."""
        with torch.no_grad():
            # (the output keywords, the statistics and the filter are refused before the stage parameters are made: that is a launch)
            output_plan(raw_u16, raw_format, raw_width, (3,), sharpen, warp, out_size, out_window, resample, out_format, yuv_matrix,
                        reverse_channels, out)
            stats_plan(raw_u16, raw_format, raw_width, (3,), statistics)
            temporal_plan(raw_u16, raw_format, raw_width, (3,), temporal_denoise)
            pars = self._stage_params(raw_u16.size(0))
            out, report = serve_reported(self.all_modules, pars, raw_u16, white_level, reverse_channels, out, black_level, cfa,
                                         fast_scene, fast_denoise, fast_cond, sharpen=sharpen, out_format=out_format,
                                         yuv_matrix=yuv_matrix, out_size=out_size, out_window=out_window, resample=resample,
                                         raw_format=raw_format, temporal_denoise=temporal_denoise, statistics=statistics, warp=warp,
                                         raw_width=raw_width, lens_shading=lens_shading, defect_correction=defect_correction,
                                         fast_median=fast_median, fast_denoise_scene=fast_denoise_scene)
            self._record(report)
        return out

    def serve_frame(self, raw_u16, white_level, patch_size, patch_stride, tile_batch=16, reverse_channels=False, out=None,
                    black_level=0, cfa='rggb', out_format='bgr8', yuv_matrix='bt601_full', sharpen=None, *, out_size=None, out_window=None,
                    resample='triangle', raw_format='u16', temporal_denoise=None, statistics=None, warp=None, raw_width=None,
                    defect_correction=None, lens_shading=None):
        """A full sensor frame through the pipeline in overlapped tiles (``pipeline_fusion.serve_frame``): (H,W) or (N,H,W)
        uint16 mosaic on the device -> (H,W,3) or (N,H,W,3) uint8, the bytes ``test_split.py`` writes for
        ``raw / white_level`` with ``patch_size`` / ``patch_stride`` (an int or a pair; H, W, sizes and strides even).  One
        ``raw_crops`` launch cuts the tiles out of the mosaic, this module's inference forward runs on slices of
        ``tile_batch`` tiles, ``risp_tile_blend_u8`` blends their last stage into the packed image: no fp32 frame at either
        end, nothing leaves the device.  ``black_level`` and ``cfa`` describe the sensor as in ``serve``.
        ``last_serve_route`` becomes 'tiled'; ``intermediate_results`` is left as it was.  ``out_format='nv12'`` and
        ``yuv_matrix`` as in ``serve``: (3H/2,W) or (N,3H/2,W), converted per frame behind the blend (``last_serve_store``
        'pass').  ``raw_format`` and ``raw_width`` as in ``serve``, (H,stride) included: unpacked once in front of the tiles
        (``last_serve_load`` 'pass').  ``lens_shading`` as in ``serve``: the whole frame is shaded once in front of the tiles
        (``last_serve_shade`` 'pass'), packed frames in that same launch.  ``defect_correction`` as in ``serve``: the whole
        frame is corrected once in front of the tiles and of the shading (``last_serve_defect`` as there), packed frames in
        that same launch.  ``temporal_denoise`` as in ``serve``: the whole frame is filtered once over its state, (H,W) being one
        image, behind those pre-passes and in front of the statistics and the tiles (``last_serve_temporal`` 'pass').
        ``out_size``, ``out_window`` and ``resample`` as in ``serve``: the frames are blended at the sensor's
        size into a cached image and one ``risp_bgr8_resize`` launch writes (OH,OW,3) or (N,OH,OW,3) - NV12 likewise -;
        ``last_serve_resize`` and ``last_serve_store`` as there.  ``statistics`` as in ``serve``: the 3A statistics of the whole
        frames, (H,W) being one image, taken once in front of the tiles (``last_serve_stats`` 'pass').  ``warp`` as in
        ``serve``: the frames are blended at the sensor's size into a cached image and one ``risp_bgr8_warp`` launch behind the
        last frame writes (WH,WW,3) or (N,WH,WW,3), in front of the resize and the NV12 conversion where those are asked for
        (``last_serve_warp`` 'pass').  ``sharpen`` as in ``serve`` (it stands in front of the ``*`` here, but is meant to be
        passed by name): one ``risp_bgr8_sharpen`` launch behind the last frame, the warp and the resize sharpens the image as
        returned, in front of the NV12 conversion (``last_serve_sharpen`` 'pass', ``last_serve_store`` as there)."""
        with torch.no_grad():
            out, report = serve_frame_reported(self.all_modules, self._stage_params, raw_u16, white_level, patch_size, patch_stride,
                                               tile_batch, reverse_channels, out, black_level, cfa, out_format, yuv_matrix, sharpen,
                                               out_size=out_size, out_window=out_window, resample=resample, raw_format=raw_format,
                                               temporal_denoise=temporal_denoise, statistics=statistics, warp=warp,
                                               raw_width=raw_width, defect_correction=defect_correction, lens_shading=lens_shading)
            self._record(report)
        return out

    def _record(self, report):
        """what the serving call recorded about itself (``pipeline_fusion.SERVE_REPORT``) -> ``last_serve_*``"""
        # (strings and None: ten trips through Module.__setattr__'s parameter and sub-module checks cost a warm call microseconds)
        self.__dict__.update(('last_serve_' + key, value) for key, value in report.items())

    @property
    def trainable_parameters(self):
        return self.all_params


class IspUniversal(_FixedPipeline):
    srgb_names = R.NAMES_SRGB_EXT

    def __init__(self, module_path, indiv_module_paths, architecture, **kwargs):
        """kwargs: gamma_in_channels / wb_manual_in_channels / wb_quadratic_in_channels for the
        conditional modules (options key network_G.conditional_modules)."""
        super().__init__()
        self._build(module_path, architecture, indiv_module_paths, kwargs)
