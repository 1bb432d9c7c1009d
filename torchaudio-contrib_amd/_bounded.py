"""The one bounded dict of the parameter-keyed caches (geometries, resampling banks, window tensors, ...).  A leaf module: it
imports nothing from the package, so every module of it can use it."""


class Bounded(dict):
    """A dict that holds at most ``limit + 1`` entries: storing a NEW key when it already holds more than ``limit`` clears it
    first.  Everything kept in one can be rebuilt from its key, so eviction is only ever a rebuild.  (``limit`` is the size
    that may be EXCEEDED by one, the policy these caches always had; ``_hip.cached_on(limit=N)`` keeps exactly N tables per slot,
    because its smallest bound — one DFT matrix — has to be exact.)"""
    __slots__ = ('limit',)

    def __init__(self, limit):
        dict.__init__(self)
        self.limit = limit

    def __setitem__(self, key, value):
        if len(self) > self.limit and key not in self:
            self.clear()
        dict.__setitem__(self, key, value)

    def __reduce__(self):
        # pickle fills a dict subclass through __setitem__ BEFORE it restores its state: ``limit`` has to come with the
        # constructor (a module that holds one, ``STFT._recipes``, is pickled by ``torch.save(module)`` and by spawn)
        return Bounded, (self.limit,), None, None, iter(self.items())
