"""tfpnp/trainer/mddpg: the critic (value network)."""
from .critic import ResNet_wobn  # noqa: F401
