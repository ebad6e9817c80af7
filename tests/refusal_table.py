"""A table of refused calls through the C ABI, for the tests of the entry points' host side
(test_gpu_side_entry_points.py, test_gpu_engine_entry_points.py): one call per fault, each asserting the return code
and the whole text of range_last_error()."""
INVALID, STATE = -1, -3


class RefusalTable:
    def __init__(self):
        self.table = []

    def rows(self, fn, ok, *faults, code=INVALID):
        """``faults``: (what, {argument index: value}, message) - ``ok`` with exactly those arguments replaced;
        the call must return ``code`` with that message."""
        for what, change, msg in faults:
            args = list(ok)
            for i, v in change.items():
                args[i] = v
            self.table.append((fn, what, args, code, msg))

    def __len__(self):
        return len(self.table)

    def check(self, lib):
        for fn, what, args, code, msg in self.table:
            rc = getattr(lib, fn)(*args)
            assert (rc, lib.range_last_error().decode()) == (code, msg), (fn, what)
