"""MI355X-native op-log composition for semmerge."""
from .ops import Op, Target  # noqa: F401
from .conflict import Conflict  # noqa: F401

__all__ = ["Op", "Target", "Conflict", "compose_oplogs", "compose_many", "compose_against",
           "compose_pairs", "compose_train", "compose_tree", "screen_conflicts", "screen_all", "screen_train",
           "screen_tree"]


def __getattr__(name):
    # compose_oplogs needs the HIP library; import lazily so schema users do not.
    if name == "compose_oplogs":
        from .compose import compose_oplogs
        return compose_oplogs
    if name == "compose_many":
        from .compose import compose_many
        return compose_many
    if name == "compose_against":
        from .compose import compose_against
        return compose_against
    if name == "compose_pairs":
        from .compose import compose_pairs
        return compose_pairs
    if name == "compose_train":
        from .compose import compose_train
        return compose_train
    if name == "compose_tree":
        from .compose import compose_tree
        return compose_tree
    if name == "screen_conflicts":
        from .compose import screen_conflicts
        return screen_conflicts
    if name == "screen_all":
        from .compose import screen_all
        return screen_all
    if name == "screen_train":
        from .compose import screen_train
        return screen_train
    if name == "screen_tree":
        from .compose import screen_tree
        return screen_tree
    raise AttributeError(name)
