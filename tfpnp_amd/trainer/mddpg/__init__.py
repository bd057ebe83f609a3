"""tfpnp/trainer/mddpg: the critic (value network) and the trainer."""
from .critic import ResNet_wobn  # noqa: F401


def __getattr__(name):
    # lazily: trainer.py needs utils.misc, which itself imports this package for the critic
    if name == "MDDPGTrainer":
        from .trainer import MDDPGTrainer
        return MDDPGTrainer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
