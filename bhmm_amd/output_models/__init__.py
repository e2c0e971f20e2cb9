from .outputmodel import OutputModel  # noqa: F401
from .gaussian import GaussianOutputModel  # noqa: F401
from .discrete import DiscreteOutputModel  # noqa: F401
from .mvgaussian import MultivariateGaussianOutputModel  # noqa: F401
from .gaussian_mixture import GaussianMixtureOutputModel  # noqa: F401
from .poisson import PoissonOutputModel  # noqa: F401
