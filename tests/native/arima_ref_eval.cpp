// Straight-line C restatement of ARIMAModel.logLikelihoodCSSARMA (S/models/ARIMA.scala:278-293
// over iterateARMA :426-463) and gradientlogLikelihoodCSSARMA (:312-381), written from the Scala
// with the reference's own data structures (the yHat vector, the maTerms array, the full
// (q + 1) x n dEdTheta matrix and its row shift).  It shares no code with the engine's
// evaluation (csrc/sts_arima_eval.hpp): tests/test_arima.py checks it bit for bit against the
// pure-Python restatement in tests/arima_ref.py and then uses it to drive that module's
// straight-line optimizer at C speed.  Build: g++ -O2 -ffp-contract=off -shared -fPIC, linked
// with the oracle for fdlibm's log.  Test infrastructure only.
#include <cstddef>
#include <cstdint>
#include <vector>

extern "C" double orc_fdlibm_log(double x);

namespace {

void update_ma_errors(std::vector<double>& errs, double new_error) {
    const int n = (int)errs.size();
    for (int i = 0; i < n - 1; i++) errs[i + 1] = errs[i];
    if (n > 0) errs[0] = new_error;
}

}  // namespace

extern "C" double aref_loglik(int p, int q, int has_intercept, const double* coefficients, const double* diffedY,
                              int n) {
    std::vector<double> yHat((std::size_t)n, 0.0), maTerms((std::size_t)q, 0.0);
    const int intercept = has_intercept ? 1 : 0;
    const int maxLag = p > q ? p : q;
    for (int i = maxLag; i < n; i++) {
        int j = 0;
        yHat[i] = yHat[i] + intercept * coefficients[j];
        while (j < p && i - j - 1 >= 0) {
            yHat[i] = yHat[i] + diffedY[i - j - 1] * coefficients[intercept + j];
            j++;
        }
        for (j = 0; j < q; j++) yHat[i] = yHat[i] + maTerms[j] * coefficients[intercept + p + j];
        update_ma_errors(maTerms, diffedY[i] - yHat[i]);
    }
    double css = 0.0;
    for (int i = maxLag; i < n; i++) {
        const double e = diffedY[i] - yHat[i];
        css += e * e;
    }
    const double sigma2 = css / n;
    return (-n / 2) * orc_fdlibm_log(2 * 3.141592653589793 * sigma2) - css / (2 * sigma2);
}

extern "C" void aref_gradient(int p, int q, int has_intercept, const double* coefficients, const double* diffedY, int n,
                              double* out) {
    const int intercept = has_intercept ? 1 : 0;
    const int nc = intercept + p + q;
    const int maxLag = p > q ? p : q;
    std::vector<double> yHat((std::size_t)n, 0.0), maTerms((std::size_t)q, 0.0), gradient((std::size_t)nc, 0.0);
    std::vector<std::vector<double>> dEdTheta((std::size_t)q + 1, std::vector<double>((std::size_t)nc, 0.0));
    double sigma2 = 0.0;
    for (int i = maxLag; i < n; i++) {
        for (int j = 0; j < nc; j++)
            for (int k = 0; k < q; k++) dEdTheta[0][j] -= coefficients[intercept + p + k] * dEdTheta[k + 1][j];
        int j = 0;
        yHat[i] += intercept * coefficients[j];
        dEdTheta[0][0] -= intercept;
        while (j < p && i - j - 1 >= 0) {
            yHat[i] += diffedY[i - j - 1] * coefficients[intercept + j];
            dEdTheta[0][intercept + j] -= diffedY[i - j - 1];
            j++;
        }
        for (j = 0; j < q; j++) {
            yHat[i] += maTerms[j] * coefficients[intercept + p + j];
            dEdTheta[0][intercept + p + j] -= maTerms[j];
        }
        const double error = diffedY[i] - yHat[i];
        sigma2 += error * error / n;
        update_ma_errors(maTerms, error);
        for (j = 0; j < nc; j++) gradient[j] += dEdTheta[0][j] * error;
        for (int r = q; r >= 1; r--) dEdTheta[r] = dEdTheta[r - 1];   // rows move back by one
        for (j = 0; j < nc; j++) dEdTheta[0][j] = 0.0;
    }
    for (int j = 0; j < nc; j++) out[j] = gradient[j] / -sigma2;
}
