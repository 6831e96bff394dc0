"""Cross-batch memory (XBM): a FIFO of the last `capacity` (image, caption) embeddings of the training steps, detached, with the
image id of every pair.  The step scores its batch against the memory as well (ops.xbm_hinge_loss / ops.xbm_infonce_loss), so one
process sees thousands of negatives.  Not part of a checkpoint: embeddings belong to the weights that made them."""
import torch

from . import ops


class MemoryBank(object):
    """Two fp32 row tables `img` [M, ...] and `cap` [M, D], allocated at the first push from the pushed shapes, and `group` [M]
    (int32).  Rows are written at the head and wrap around; view() shows the filled slots in STORAGE order (the order the losses'
    tie rule sees), not in order of age."""

    def __init__(self, capacity, device):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("MemoryBank: capacity must be at least 1, got %d" % capacity)
        self.capacity = capacity
        self.device = torch.device(device)
        self.img = self.cap = self.group = None
        self.head = 0          # slot of the next row
        self.pushed = 0        # rows pushed since the last reset()

    def __len__(self):
        return min(self.pushed, self.capacity)

    def reset(self):
        """Empty the memory (the tables stay allocated)."""
        self.head = 0
        self.pushed = 0

    def push(self, img, cap, groups):
        """Append B detached rows: one launch of the ring-write kernel per table."""
        img, cap = img.detach(), cap.detach()
        B = img.shape[0]
        if cap.shape[0] != B:
            raise ValueError("MemoryBank.push: %d image rows but %d caption rows" % (B, cap.shape[0]))
        if B > self.capacity:
            raise ValueError("MemoryBank.push: %d rows do not fit a memory of %d" % (B, self.capacity))
        for name, t in (("img", img), ("cap", cap)):
            if not t.is_cuda or t.dtype != torch.float32:
                raise TypeError("MemoryBank.push: %s must be a float32 device tensor, got %s on %s" % (name, t.dtype, t.device))
        groups = ops._hinge_groups(groups, B, self.device)
        if self.img is None:
            self.img = torch.zeros((self.capacity,) + tuple(img.shape[1:]), device=self.device, dtype=torch.float32)
            self.cap = torch.zeros((self.capacity,) + tuple(cap.shape[1:]), device=self.device, dtype=torch.float32)
            self.group = torch.zeros(self.capacity, device=self.device, dtype=torch.int32)
        if img.shape[1:] != self.img.shape[1:] or cap.shape[1:] != self.cap.shape[1:]:
            raise ValueError("MemoryBank.push: rows of %s / %s do not match the tables %s / %s" % (
                tuple(img.shape), tuple(cap.shape), tuple(self.img.shape), tuple(self.cap.shape)))
        if B:
            ops.xbm_ring_write(img, self.img, self.head)
            ops.xbm_ring_write(cap, self.cap, self.head)
            ops.xbm_ring_write(groups, self.group, self.head)
        self.head = (self.head + B) % self.capacity
        self.pushed += B

    def view(self):
        """-> (img[:n], cap[:n], group[:n]), n = min(pushed, capacity); views of the tables, in storage order."""
        n = len(self)
        if self.img is None:
            raise ValueError("MemoryBank.view: nothing was pushed yet")
        return self.img[:n], self.cap[:n], self.group[:n]
