"""The batch buffers the stager tests hand to the stager (tests/test_integration.py,
tests/test_hip_stager_reuse.py)."""
import ctypes

import numpy as np

import aeon_amd as A


class Buffer:
    """One buffer_fixed_size_elements of a batch (src/buffer_batch.hpp:154-188): pageable numpy,
    pinned host (aeon's "pinned" loader option: buffer_fixed_size_elements::allocate's HAS_GPU branch,
    src/buffer_batch.cpp:150-186, as INTEGRATION.md edit 5 rewrites it -- aeon_hip_host_alloc /
    aeon_hip_host_free) or device memory."""

    def __init__(self, nbytes, where):
        import torch
        self.where = where
        if where == "device":
            self.t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            self.ptr = self.t.data_ptr()
        elif where == "pinned":
            p = ctypes.c_void_p()
            A._check(A.lib().aeon_hip_host_alloc(nbytes, ctypes.byref(p)))
            self.ptr, self.n = p.value, nbytes
            ctypes.memset(self.ptr, 0, nbytes)
        else:
            self.a = np.zeros(nbytes, np.uint8)
            self.ptr = self.a.ctypes.data

    def bytes(self):
        if self.where == "device":
            return self.t.cpu().numpy()
        if self.where == "pinned":
            return np.ctypeslib.as_array((ctypes.c_uint8 * self.n).from_address(self.ptr)).copy()
        return self.a

    def free(self):
        if self.where == "pinned":
            A.lib().aeon_hip_host_free(ctypes.c_void_p(self.ptr))
