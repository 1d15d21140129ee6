"""The layout of the operator modules (host only): ops.py is the shared core and re-exports every family's public operators;
a family module reaches the core as ops.NAME at call time (the access rule at the top of ops.py)."""
import ast
import pathlib

import sisr_amd

PACKAGE = pathlib.Path(sisr_amd.__file__).parent

# every public attribute of ops (modules aside) when the operators were split into family modules: callers say ops.NAME
PUBLIC = """
    BATCH_WGRAD BATCH_WGRAD_JOBS BATCH_WGRAD_MAX_PIXELS BF16_STORAGE CL FUSED_GROUPS FrozenChain Function GATE_HEADS
    GATE_HEADS_MAX_PIXELS GRAD_SINK IN_BACKWARD LANES LEAKY LEAKY_MASK MS_SSIM_MAX_LEVELS MS_SSIM_WEIGHTS PRECISION
    QCA_STYLES REFL_BATCH REFL_GEO SELECT_WINOGRAD SELECT_WINOGRAD_FORCE SELECT_WINOGRAD_PREDICATED SOCA_ITERS
    SOCA_LIMIT SPARSE_BLOCK_DIAGONAL SPARSE_HALVES SPARSE_SECOND_CHUNK SPECTRAL_MAX_SIDE SPECTRAL_MIN_SIDE
    SPECTRAL_TABLE_SLOTS SSIM_WINDOW WGRAD_SIDE_STREAM WINOGRAD_FLOATS WgradGeoQueue WgradQueue X3_WGRAD add_residual
    batch_norm_act ca_layer conv3x3 conv3x3_stack conv_1x1 conv_c64 conv_c64s conv_chain conv_f2y conv_kxk conv_kxk_s2
    conv_s2_out_size conv_y2f convk_mfma convk_mfma_leaky csam deferred_wgrads frozen_features fused_groups_enabled
    gap_parts gate_mul gated_group global_avg_pool group_norm instance_norm_act invalidate_packs l1_loss lam leaky_relu
    map_mean meta_gate meta_gate_many ms_ssim_check_size ms_ssim_mean ms_ssim_min_side ms_ssim_weights mse_loss
    nchw_to_nhwc_pad nearest_up nonlocal_attention nonlocal_block pa_layer pack_all pack_convk pack_pair pack_weight
    pad_param pixel_norm pixel_shuffle prelu qca_gate refl_conv res_block res_block_convs scale_add selu set_precision
    set_storage sft_apply sft_layer sftmd_forward shuffle_rgb side_stream soca soca_window spar_combine spar_combine3d
    spectral_l1 spectral_tables ssim_mean stack_maps to_bf16_map wgrad_c64
""".split()


def test_no_module_binds_names_of_ops_at_import_time():
    """`from .ops import NAME` copies a value: bench.py, the tools and the tests replace ops.conv_c64 / ops.wgrad_c64 and flip
    ops' switches while a step runs, and the copy would not follow"""
    files = sorted(p for p in PACKAGE.glob("*.py") if p.name != "ops.py")
    assert len(files) > 25
    bound = [f"{p.name}:{n.lineno}" for p in files for n in ast.walk(ast.parse(p.read_text(encoding="utf-8")))
             if isinstance(n, ast.ImportFrom) and n.level == 1 and n.module == "ops"]
    assert not bound, f"`from .ops import ...` in {bound}: reach the core as ops.NAME at call time"


def test_ops_still_offers_every_public_name():
    assert len(PUBLIC) == 112
    missing = [n for n in PUBLIC if not hasattr(sisr_amd.ops, n)]
    assert not missing, f"ops no longer offers {missing}"
