"""cdist_standin's stand-in library with K28's entry recorded like K27's -- a helper for test_cdprof_host.py, no tests here.
standin_lib.py and cdist_standin.py stay as they are."""
import cdist_standin as ST

K28 = 'xc_contour_distance_profile_dev'


class Lib(ST.Lib):
    """cdist_standin's `Lib`, and xc_contour_distance_profile_dev recorded with its nrange (argument 1), scripted through `on`"""

    def __getattr__(self, name):
        if name == K28:
            return lambda *a: self._record28(a)
        return ST.Lib.__getattr__(self, name)

    def _record28(self, a):
        self.calls.append((K28, int(a[1])))
        self.args.append((K28, tuple(a)))
        return self.on[K28](self, a) if K28 in self.on else 0
