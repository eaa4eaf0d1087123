"""In-tree build of the gfx950 HIP extension.

Usage:
    PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace

Produces msrflute_amd/_C.*.so next to the package sources so the built
artifact travels with the tree (no JIT cache dependence).
"""

import os
import subprocess

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

from setuptools import setup
from torch.utils.cpp_extension import (ROCM_HOME, BuildExtension,
                                       CUDAExtension)

ROOT = os.path.dirname(os.path.abspath(__file__))
HIP_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950"]

ext = CUDAExtension(
    name="msrflute_amd._C",
    sources=[
        "msrflute_amd/csrc/bindings.cpp",
        "msrflute_amd/csrc/flat_ops.hip",
        "msrflute_amd/csrc/fused_cnn.hip",
        "msrflute_amd/csrc/lstm_seq.hip",
        "msrflute_amd/csrc/gru_seq.hip",
    ],
    extra_compile_args={"cxx": ["-O3", "-std=c++17"], "nvcc": HIP_FLAGS},
)


class Build(BuildExtension):
    """gru_seq_bf16.hip (the bf16 instantiation of the GRU kernels, nothing
    else) is compiled on its own, without gfx950's packed fp32 VALU ops:
    measured, its forward is 9 % faster that way and the pair 3 %
    (profiles/r07_gru_bf16_stats.md).  The flag is a whole-file one and an
    extension's flags are shared by all its sources, so the object is made
    here and handed to the link.  Every other source, the fp32 GRU kernels
    in gru_seq.hip included, is built by torch with the flags above.

    The any-H GRU pair (gru_seq_any.hip) is built the same way: its scalar
    fmaf chains are the design, and the compile figures and times recorded
    in docs/kernels.md are those of the code without packed pairs.  So is
    the short-sequence attention pair (mha_small.hip), for the same reason:
    four scalar fmaf chains per dot product in a fixed order.  The
    attentive pooling pair (attn_pool.hip) joins them: its matrix work is
    on the MFMA pipe, what is left are scalar fmaf chains in a fixed order,
    and its tanh / exp (scalar_math.h) are the code the LSTM kernels
    compile without packed pairs.  So does the title convolution pair
    (conv1d_seq.hip): MFMA chains and a scalar bias / max epilogue.  Its
    backward-weights pair (conv1d_bwd_w.hip) is MFMA chains, a scalar db
    chain and a fold whose adds run in a fixed order.  The MFMA attention
    pair (mha_mfma.hip) is MFMA chains and a scalar softmax in a fixed
    order, with scalar_math.h's exp."""

    NO_PACKED_FP32 = ("gru_seq_bf16", "gru_seq_any", "mha_small",
                      "attn_pool", "conv1d_seq", "conv1d_bwd_w", "mha_mfma")

    def build_extensions(self):
        os.makedirs(self.build_temp, exist_ok=True)
        for stem in self.NO_PACKED_FP32:
            src = os.path.join(ROOT, "msrflute_amd", "csrc", stem + ".hip")
            obj = os.path.join(self.build_temp, stem + ".o")
            subprocess.check_call(
                [os.path.join(ROCM_HOME, "bin", "hipcc"), "-c", src, "-o",
                 obj, "-fPIC", "-fno-gpu-rdc", *HIP_FLAGS,
                 "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"])
            self.extensions[0].extra_objects.append(obj)
        super().build_extensions()

setup(
    name="msrflute_amd",
    version="0.1.0",
    packages=["msrflute_amd"],
    ext_modules=[ext],
    cmdclass={"build_ext": Build.with_options(no_python_abi_suffix=False)},
)
