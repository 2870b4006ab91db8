from .minimal import Minimal  # noqa: F401
from .explorer import Explorer  # noqa: F401
from .deathmatch import Deathmatch  # noqa: F401
from .pointgoal import PointGoal  # noqa: F401
from .floorcoverage import FloorCoverage  # noqa: F401
from .patrol import Patrol  # noqa: F401
from .tag import Tag  # noqa: F401
from .forage import Forage  # noqa: F401
