// instantiate_all.cpp -- every public function template of include/dlaf_mi355x/dlaf.hpp (and its three class templates),
// explicitly instantiated for float, double, std::complex<float> and std::complex<double>: every overload, grid and local,
// host- and device-resident.  Nothing runs: compiling proves that each signature exists as written here, linking proves
// that the C entry each instantiation names exists in the library for that element type.
#include <complex>
#include <utility>
#include <vector>

#include <dlaf_mi355x/dlaf.hpp>

using namespace dlaf;
using Grid = comm::CommunicatorGrid;
template <class T>
using Host = Matrix<T, Device::CPU>;
template <class T>
using Dev = Matrix<T, Device::GPU>;
template <class T>
using Vec = std::vector<T>;
template <class T>
using Getter = T (*)(const GlobalElementIndex&);
using Range = std::pair<SizeType, SizeType>;
using blas::Diag;
using blas::Op;
using blas::Side;
using blas::Uplo;
using lapack::Norm;
constexpr Backend G = Backend::GPU;
constexpr Device C = Device::CPU;

#define INSTANTIATE(T)                                                                                                     \
  template class dlaf::Matrix<T, Device::CPU>;                                                                             \
  template class dlaf::Matrix<T, Device::GPU>;                                                                             \
  template class dlaf::matrix::MatrixMirror<T, Device::GPU, Device::CPU>;                                                  \
  template void dlaf::matrix::util::set<T, Getter<T>>(Host<T>&, Getter<T>&&);                                              \
  template void dlaf::matrix::util::set_random_hermitian_positive_definite<T>(const Grid&, Host<T>&);                      \
                                                                                                                           \
  template void dlaf::cholesky_factorization<G, Device::GPU, T>(Grid&, Uplo, Dev<T>&);                                     \
  template void dlaf::cholesky_factorization<G, C, T>(Grid&, Uplo, Host<T>&);                                              \
  template void dlaf::cholesky_factorization<G, C, T>(Uplo, Host<T>&);                                                     \
  template void dlaf::triangular_solver<G, C, T>(Grid&, Side, Uplo, Op, Diag, T, Host<T>&, Host<T>&);                      \
  template void dlaf::triangular_solver<G, C, T>(Side, Uplo, Op, Diag, T, Host<T>&, Host<T>&);                             \
  template void dlaf::triangular_multiplication<G, C, T>(Grid&, Side, Uplo, Op, Diag, T, Host<T>&, Host<T>&);              \
  template void dlaf::triangular_multiplication<G, C, T>(Side, Uplo, Op, Diag, T, Host<T>&, Host<T>&);                     \
  template void dlaf::hermitian_multiplication<G, C, T>(Grid&, Side, Uplo, T, const Host<T>&, const Host<T>&, T, Host<T>&); \
  template void dlaf::hermitian_multiplication<G, C, T>(Side, Uplo, T, const Host<T>&, const Host<T>&, T, Host<T>&);       \
  template void dlaf::multiplication::internal::generalMatrix<G, C, T>(Grid&, Op, Op, T, const Host<T>&, const Host<T>&,   \
                                                                       T, Host<T>&);                                       \
  template void dlaf::multiplication::internal::generalMatrix<G, C, T>(Op, Op, T, const Host<T>&, const Host<T>&, T,       \
                                                                       Host<T>&);                                          \
  template void dlaf::multiplication::internal::generalMatrix<G, C, T>(Grid&, T, const Host<T>&, const Host<T>&, T,        \
                                                                       Host<T>&);                                          \
  template void dlaf::hermitian_rank_k_update<G, C, T>(Grid&, Uplo, Op, BaseType<T>, const Host<T>&, BaseType<T>,          \
                                                       Host<T>&);                                                          \
  template void dlaf::hermitian_rank_k_update<G, C, T>(Uplo, Op, BaseType<T>, const Host<T>&, BaseType<T>, Host<T>&);      \
  template void dlaf::hermitian_rank_2k_update<G, C, T>(Grid&, Uplo, Op, T, const Host<T>&, const Host<T>&, BaseType<T>,   \
                                                        Host<T>&);                                                         \
  template void dlaf::hermitian_rank_2k_update<G, C, T>(Uplo, Op, T, const Host<T>&, const Host<T>&, BaseType<T>,          \
                                                        Host<T>&);                                                         \
  template void dlaf::hermitian_weighted_rank_k_update<G, C, T>(Grid&, Uplo, Op, BaseType<T>, const Host<T>&,              \
                                                                const BaseType<T>*, BaseType<T>, Host<T>&);                \
  template void dlaf::hermitian_weighted_rank_k_update<G, C, T>(Uplo, Op, BaseType<T>, const Host<T>&, const BaseType<T>*, \
                                                                BaseType<T>, Host<T>&);                                    \
  template int dlaf::hermitian_function<G, C, T>(Grid&, Uplo, Host<T>&, BaseType<T>*,                                      \
                                                 const SpectralWeights<BaseType<T>>&, SpectralSelection<BaseType<T>>,      \
                                                 SizeType*);                                                               \
  template int dlaf::hermitian_power<G, C, T>(Grid&, Uplo, Host<T>&, BaseType<T>*, double, double, SizeType*);             \
  template void dlaf::general_addition<G, C, T>(Grid&, Uplo, Op, T, const Host<T>&, T, Host<T>&);                          \
  template void dlaf::general_addition<G, C, T>(Uplo, Op, T, const Host<T>&, T, Host<T>&);                                 \
  template void dlaf::hermitian_complete<G, C, T>(Grid&, Uplo, bool, Host<T>&);                                            \
  template void dlaf::hermitian_complete<G, C, T>(Uplo, bool, Host<T>&);                                                   \
                                                                                                                           \
  template void dlaf::eigensolver::internal::generalized_to_standard<G, T>(Grid&, Uplo, Host<T>&, Host<T>&);               \
  template void dlaf::eigensolver::internal::generalized_to_standard<G, T>(Grid&, Uplo, Dev<T>&, Dev<T>&);                 \
  template void dlaf::eigensolver::internal::generalized_to_standard<G, T>(Uplo, Host<T>&, Host<T>&);                      \
  template int dlaf::triangular_inverse<G, T>(Grid&, Uplo, Diag, Host<T>&);                                                \
  template int dlaf::triangular_inverse<G, T>(Grid&, Uplo, Diag, Dev<T>&);                                                 \
  template int dlaf::triangular_inverse<G, T>(Uplo, Diag, Host<T>&);                                                       \
  template int dlaf::inverse_from_cholesky_factor<G, T>(Grid&, Uplo, Host<T>&);                                            \
  template int dlaf::inverse_from_cholesky_factor<G, T>(Grid&, Uplo, Dev<T>&);                                             \
  template int dlaf::inverse_from_cholesky_factor<G, T>(Uplo, Host<T>&);                                                   \
                                                                                                                           \
  template BaseType<T> dlaf::auxiliary::norm<G, T>(Grid&, Norm, Host<T>&);                                                 \
  template BaseType<T> dlaf::auxiliary::norm<G, T>(Grid&, Norm, Uplo, Host<T>&);                                           \
  template BaseType<T> dlaf::auxiliary::norm<G, T>(Grid&, Norm, Uplo, Dev<T>&);                                            \
  template BaseType<T> dlaf::auxiliary::norm<G, T>(Grid&, Norm, Uplo, Diag, Host<T>&);                                     \
  template BaseType<T> dlaf::auxiliary::norm<G, T>(Grid&, Norm, Uplo, Diag, Dev<T>&);                                      \
  template BaseType<T> dlaf::auxiliary::max_norm<G, Device::CPU, T>(Grid&, comm::Index2D, Uplo, Host<T>&);                 \
  template BaseType<T> dlaf::auxiliary::max_norm<G, Device::GPU, T>(Grid&, comm::Index2D, Uplo, Dev<T>&);                  \
                                                                                                                           \
  template Vec<T> dlaf::eigensolver::internal::reduction_to_band<G, T>(Grid&, Dev<T>&, SizeType);                          \
  template Vec<T> dlaf::eigensolver::internal::reduction_to_band<G, T>(Grid&, Host<T>&, SizeType);                         \
  template Vec<T> dlaf::eigensolver::internal::reduction_to_band<G, T>(Host<T>&, SizeType);                                \
  template void dlaf::eigensolver::internal::bt_reduction_to_band<G, T>(Grid&, SizeType, Host<T>&, Host<T>&,               \
                                                                        const Vec<T>&);                                    \
  template void dlaf::hermitian_eigensolver<G, T>(Grid&, Uplo, Host<T>&, Vec<BaseType<T>>&, Host<T>&);                     \
  template void dlaf::hermitian_eigensolver<G, T>(Grid&, Uplo, Host<T>&, Vec<BaseType<T>>&, Host<T>&, SizeType, SizeType); \
  template Range dlaf::hermitian_eigensolver<G, T>(Grid&, Uplo, Host<T>&, Vec<BaseType<T>>&, Host<T>&,                     \
                                                   EigenvaluesValue<BaseType<T>>);                                         \
  template void dlaf::hermitian_generalized_eigensolver<G, T>(Grid&, Uplo, Host<T>&, Host<T>&, Vec<BaseType<T>>&,          \
                                                              Host<T>&);                                                   \
  template void dlaf::hermitian_generalized_eigensolver<G, T>(Grid&, Uplo, Host<T>&, Host<T>&, Vec<BaseType<T>>&,          \
                                                              Host<T>&, SizeType, SizeType);                               \
  template Range dlaf::hermitian_generalized_eigensolver<G, T>(Grid&, Uplo, Host<T>&, Host<T>&, Vec<BaseType<T>>&,         \
                                                               Host<T>&, EigenvaluesValue<BaseType<T>>);                   \
  template void dlaf::hermitian_eigenvalues<G, T>(Grid&, Uplo, const Host<T>&, Vec<BaseType<T>>&, SizeType, SizeType);     \
  template void dlaf::hermitian_generalized_eigenvalues<G, T>(Grid&, Uplo, const Host<T>&, Host<T>&, Vec<BaseType<T>>&,    \
                                                              SizeType, SizeType);

INSTANTIATE(float)
INSTANTIATE(double)
INSTANTIATE(std::complex<float>)
INSTANTIATE(std::complex<double>)

int main() {}
