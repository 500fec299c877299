"""define_G(opt) - which_model_G -> pipeline graph (mirror of models/networks.py:10-48).

The reference hard-codes ``module_path = '/DATA/module/'``; that stays the default, and the
optional key ``network_G.module_path`` overrides it (``~``/None = no weight files: proxies keep
their random initialisation - used by the synthetic benchmark and the tests)."""
import logging

logger = logging.getLogger('base')
DEFAULT_MODULE_PATH = '/DATA/module/'


def demosaicnet_options(opt_net):
    """(weights path or None, cfa phase) of the optional keys network_G.demosaicnet_weights / demosaicnet_cfa (default 'rggb')"""
    path = opt_net['demosaicnet_weights'] if 'demosaicnet_weights' in opt_net else None
    cfa = opt_net['demosaicnet_cfa'] if 'demosaicnet_cfa' in opt_net and opt_net['demosaicnet_cfa'] else 'rggb'
    return (path or None), cfa


def define_G(opt):
    opt_net = opt['network_G']
    # DemosaicNet (demosaic index 04) is unavailable unless weights are given: then the built-in HIP implementation is registered
    # for every network kind (the super-net stops masking the op, the fixed pipelines can evaluate Demosaic_04)
    dmnet_path, dmnet_cfa = demosaicnet_options(opt_net)
    if dmnet_path is not None:
        from ...isp_kernels import demosaic as _dm
        _dm.load_demosaicnet(dmnet_path, dmnet_cfa)
        logger.info('DemosaicNet: weights %s (cfa %s)', dmnet_path, dmnet_cfa)
    module_path = opt_net['module_path'] if 'module_path' in opt_net else DEFAULT_MODULE_PATH
    which = opt_net['which_model_G']

    if which == 'SuperPruneFifteenDemosFourBayerTwo':
        from .modules.super_prune_fifteen_demos_four_bayer_two import SuperPruneFifteenDemosFourBayerTwo
        opt_net['n_modules']  # read (and required) by the reference, unused there too (networks.py:23)
        return SuperPruneFifteenDemosFourBayerTwo(n_step=opt_net['n_step'], threshold=opt_net['prune_threshold'],
                                                  module_path=module_path)
    if which == 'SuperPruneFifteenDemosFourBayerTwoFt':
        from .modules.super_prune_fifteen_demos_four_bayer_two_ft import SuperPruneFifteenDemosFourBayerTwoFt
        opt_net['n_modules']
        return SuperPruneFifteenDemosFourBayerTwoFt(n_step=opt_net['n_step'], threshold=opt_net['prune_threshold'],
                                                    module_path=module_path)
    if which == 'IspUniversal':
        from .modules.isp_universal import IspUniversal
        cond = opt_net['conditional_modules'] if 'conditional_modules' in opt_net else {}
        return IspUniversal(module_path=module_path, indiv_module_paths=opt_net['individual_module_paths'],
                            architecture=opt_net['architecture'], **(cond or {}))
    if which == 'OriginUniversal':
        from .modules.origin_universal import OriginUniversal
        classical_bm3d = bool(opt_net['classical_bm3d']) if 'classical_bm3d' in opt_net else False
        return OriginUniversal(module_path=module_path, architecture=opt_net['architecture'], classical_bm3d=classical_bm3d)
    raise NotImplementedError('Generator model [{:s}] not recognized'.format(which))
