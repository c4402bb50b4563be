"""standin_lib's stand-in library with K27's entry recorded like the other record kernels -- a helper for test_cdist_host.py, no tests
here.  standin_lib.py itself stays as it is."""
import standin_lib as SL

K27 = 'xc_contour_distance_dev'


class Lib(SL._Lib):
    """`_Lib`, and xc_contour_distance_dev recorded with its nrange (argument 1), scripted through `on` like every other entry"""

    def __getattr__(self, name):
        if name == K27:
            return lambda *a: self._record27(a)
        return SL._Lib.__getattr__(self, name)

    def _record27(self, a):
        self.calls.append((K27, int(a[1])))
        self.args.append((K27, tuple(a)))
        return self.on[K27](self, a) if K27 in self.on else 0
