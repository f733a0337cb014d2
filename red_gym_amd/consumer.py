"""What the step's consumers share.  A consumer is a kernel enqueued behind every step that adds keys to `info`: the progress
tracker (progress.py), the reward shaper (shaping.py), the path follower (pathfollow.py), the replay buffer (replay.py) and the
episode tracker (episodes.py).  The
Engine owns one object of each; F110VecEnv loops over them."""
import ctypes as C
import weakref

import torch

from . import _lib


class Consumer(object):
    """Nothing is allocated before the first install().  A subclass names its entry points (NAME: f110_<NAME>_bind / _update)
    and gives INFO (`info` key -> buffer name), STATE (state_dict key -> buffer name), install(), remove() and restart().
    `buf` holds its tensors by name, `info` the views that join the step's `info` while it is `on`."""
    reward = None   # the reward [B] the consumer pays (None: the env's constant stays)

    def __init__(self, eng):
        self.eng = weakref.proxy(eng)   # (the Engine owns this object: a strong reference would keep both alive until a GC cycle)
        self.on, self.buf, self.info = False, None, {}
        self._update = getattr(eng.lib, 'f110_%s_update' % self.NAME)

    def _bind(self, buf, struct, fields=None):
        """The tensors `buf` become the buffers the kernel writes: one struct of pointers, handed to the library once.
        `fields`: struct field -> name in `buf` where the two differ, None for a field that stays NULL."""
        ptrs = struct()
        for name, _ in struct._fields_:
            key = (fields or {}).get(name, name)
            setattr(ptrs, name, None if key is None else buf[key].data_ptr())
        torch.cuda.synchronize(self.eng.device)
        _lib.check(getattr(self.eng.lib, 'f110_%s_bind' % self.NAME)(self.eng._h, C.byref(ptrs)))
        self.buf, self.info = buf, {k: buf[name] for k, name in self.INFO.items()}

    def kernel(self):
        """Enqueues the consumer's kernel on the current stream for the state as the last step left it (no allocation, no
        synchronisation -- it can be captured behind step()).  ValueError from the library while nothing is installed."""
        with torch.cuda.device(self.eng.device):
            _lib.check(self._update(self.eng._h, self.eng._stream()))

    update = kernel   # what follows every step

    def state(self):
        return {k: self.buf[name].clone() for k, name in self.STATE.items()}

    def load(self, sd):
        """Restores state() from a checkpoint that holds this consumer's keys with fitting shapes; any other restarts it."""
        if all(k in sd and sd[k].shape == self.buf[name].shape for k, name in self.STATE.items()):
            for k, name in self.STATE.items():
                self.buf[name].copy_(sd[k])
        else:
            self.restart()

    def state_keys(self):
        """Every state_dict key that is this consumer's, whether it would load it or not."""
        return set(self.STATE)

    def on_load_state_dict(self, sd):
        """What F110VecEnv.load_state_dict asks of a consumer that is `on`."""
        self.load(sd)

    def close(self):
        pass
