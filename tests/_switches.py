"""The schedule switches (GSX_*: README) for tests.  A handle reads them once, when it is created, and keeps them for its
life: make the handle inside `with switches(GSX_X="0"):`, use it anywhere."""
import contextlib
import os


@contextlib.contextmanager
def switches(**env):
    """Set the given environment variables (None: unset), yield, and put back what was there."""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
