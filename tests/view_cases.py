"""Channel-slice views for the kernel tests (a helper, not a test module).

The engine never materialises the decoder concat: a skip tensor and the x2 upsample live in column
ranges of one wide `cat*` buffer, and kernels get them as Act(buf, off, ld, C) views whose row stride
`ld` is larger than `C` (seg_amd/engine.py; include/segamd.h promises `ld* >= round_up(C, 4)` for every
entry point).  This module holds

  * COVERAGE: the (entry point, operand role) pairs tests/test_gpu_views.py runs on such a view --
    tests/test_views_covered.py derives the pairs the production programs need and fails for one that
    is missing here;
  * make_view / guards_intact: a view inside a wider buffer whose other columns hold a fill pattern
    (NaN around an input, so a kernel reading them as data poisons its result; a finite sentinel
    around an output), and the bitwise check that the pattern survived the launch.

Roles: in / out / add (conv input, output, fused addend), x / dy (weight-gradient operands), by (the
BN layer's pre-BN output read by seg_conv_igemm_bnout*), res (residual), din (a resampling kernel's
gradient output), dout (its gradient input); x is also the input of the fused inference kernels whose
argument has that name.
"""
import torch

NAN = float("nan")
SENTINEL = 7.0  # finite, exact in fp32, bf16 and fp16


def _pairs(table):
    return sorted({(name, role) for names, roles in table for name in names.split() for role in roles.split()})


# entry points (space separated) x the roles test_gpu_views.py puts on a view for each of them
COVERAGE = _pairs([
    # training: thin-K 1x1 convs (test_pw_forward_views, test_pw_dgrad_views)
    ("seg_conv_pw seg_conv_pw_bf16io", "in out add"),
    # the implicit GEMM and its lazy-BN twins (test_igemm_views)
    ("seg_conv_igemm seg_conv_igemm_bf16 seg_conv_igemm_bf16io seg_conv_igemm_bf16io_w16 "
     "seg_conv_igemm_xf seg_conv_igemm_bf16_xf seg_conv_igemm_bf16io_xf seg_conv_igemm_bf16io_xf_w16", "in out add"),
    ("seg_conv_igemm2_bf16io", "in out add"),                                              # test_igemm2_views
    ("seg_conv_igemm_bnout seg_conv_igemm_bnout_bf16io seg_conv_igemm_bnout_bf16io_w16", "out add by"),   # test_bnout
    ("seg_conv_wgrad seg_conv_wgrad_bf16 seg_conv_wgrad_bf16io "
     "seg_conv_wgrad_xf seg_conv_wgrad_bf16_xf seg_conv_wgrad_bf16io_xf", "x dy"),          # test_wgrad_views
    ("seg_conv_wgrad2_bf16io seg_conv_wino_wgrad seg_conv_wino_wgrad16", "x dy"),          # test_wgrad_3x3_views
    ("seg_conv_wino seg_conv_wino_fused", "in out"),                                       # test_wino_views
    ("seg_conv_halo seg_conv_halo_bf16io seg_conv_halo_bf16io_w16", "in out"),             # test_halo_views
    ("seg_maxpool2_fwd seg_maxpool2_fwd_bf16io", "in"),                                    # test_maxpool_views
    ("seg_maxpool2_bwd seg_maxpool2_bwd_bf16io", "in din"),
    ("seg_upsample_fwd seg_upsample_fwd_bf16io", "in out"),                                # test_upsample_fwd_views
    ("seg_upsample_bwd seg_upsample_bwd_bf16io", "dout din"),                              # test_upsample_bwd_views
    # folded inference forward
    ("seg_conv_igemm_act_ic seg_conv_igemm_bf16_ic seg_conv_igemm_f16_ic", "in out add"),  # test_igemm_ic_views
    ("seg_mbconv_f16", "x out res"),                                                       # test_mbconv_views
    ("seg_pw2_f16", "x"),                                                                  # test_pw2_views
    ("seg_stem_pre_f16", "out"),                                                           # test_stem_pre_views
])


def _bits(t):
    """The tensor's bit patterns (so NaN == NaN and -0.0 != 0.0)."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def make_view(M, C, ld, off, dtype, fill, data=None, device="cuda"):
    """An [M][C] view at columns [off, off + C) of a fresh [M][ld] buffer whose other columns hold `fill`.
    Returns (the wide buffer, the pointer to the view, a contiguous copy of the view's columns).  `data`
    ([M][C]) fills the view; None leaves SENTINEL there.  As the engine makes them: C, ld and off multiples
    of a 16-byte vector, and at least one more vector of fill to the right of the view (so a kernel that
    stores one vector past its slice stays inside the buffer and is caught by guards_intact)."""
    v = 16 // torch.empty(0, dtype=dtype).element_size()
    assert C % v == 0 and ld % v == 0 and off % v == 0 and off + C + v <= ld, (C, ld, off, v)
    buf = torch.full((M, ld), fill, dtype=dtype, device=device)
    buf[:, off:off + C] = SENTINEL if data is None else data.to(device=device, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:, off:].data_ptr(), buf[:, off:off + C].contiguous()


def guards_intact(buf, off, C, fill):
    """Every column of `buf` outside [off, off + C) still holds `fill`, bit for bit."""
    want = _bits(torch.full((1,), fill, dtype=buf.dtype, device=buf.device))
    b = _bits(buf)
    return bool((b[:, :off] == want).all()) and bool((b[:, off + C:] == want).all())
