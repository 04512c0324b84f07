"""The one status path a module reaches with nothing launched: a correlation backward with stride1 != 1, which the C ABI of both
correlation libraries rejects in front of its launch.  The sibling module words it through csrc/binding/binding_status.h, the
main one through fn2_strerror."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_backward_with_stride1_2_is_rejected_in_each_librarys_words(dev):
    import correlation1d_cuda
    import correlation_cuda
    g = torch.Generator().manual_seed(5)
    a, b = (torch.randn(1, 2, 4, 8, generator=g).to(dev) for _ in range(2))
    pad_size, max_displacement, stride1, stride2 = 2, 2, 2, 1

    out = correlation1d_cuda.forward_alloc(a, b, pad_size, max_displacement, stride1, stride2, 0)
    with pytest.raises(RuntimeError, match=r"correlation1d_cuda\.backward: HIP call failed: flownet2_hip_ext: unsupported parameter combination "
                                           r"\(the backward needs stride1 == 1\) \(code -4\)"):
        correlation1d_cuda.backward_alloc(a, b, torch.ones_like(out), pad_size, max_displacement, stride1, stride2, 0)

    out = correlation_cuda.forward_alloc(a, b, pad_size, 1, max_displacement, stride1, stride2, 1)
    with pytest.raises(RuntimeError, match=r"correlation_cuda\.backward: HIP call failed: flownet2_hip: parameter combination the reference "
                                           r"leaves undefined \(code -4\)"):
        correlation_cuda.backward_alloc(a, b, torch.ones_like(out), pad_size, 1, max_displacement, stride1, stride2, 1)
    torch.cuda.synchronize()
